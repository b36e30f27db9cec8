"""Batch preparation of the stage-0 step executor (engine.Stage0Engine): the rotating ray buffers and the pipeline that keeps `depth`
batches marched ahead of the running step, on a side stream behind the step's go-ahead event."""
import torch

from . import _lib as L
from . import capture as C
from . import synthetic

_p = L.ptr


class _RayBufs:
    """Per-batch ray-side tensors.  Three sets rotate: while step i consumes batch i, batch i+1 waits for its turn and batch i+2 is
    produced on the side stream (behind the marker in front of Adam(i), i.e. after the last kernel that read batch i-1's set)."""

    def __init__(self, cap, dev):
        self.cap = cap
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        self.o, self.d, self.rgba = f(cap, 3), f(cap, 3), f(cap, 4)
        self.nears, self.fars, self.noises, self.bg_buf = f(cap), f(cap), f(cap), f(cap, 3)
        self.gtd, self.dw = f(cap), f(cap)      # keypoint depth and weight of a depth batch (capture.batch_sparse_u8)
        self.depth_view = None                  # the view of a depth batch, None for a plain one
        self.u = self.bg = None
        self.rays = torch.empty(cap, 2, dtype=torch.int32, device=dev)
        self.views = None            # int32 [cap]: the view of every ray (individual codes only: BatchPipeline.prepare allocates it)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ws = torch.empty(int(L.lib().n2m_march_fused_workspace_bytes(cap)), dtype=torch.uint8, device=dev)   # chunk records, group totals
        self.one_pass = False        # samples written by the single-pass marcher (complete once the count is)
        self.host_count = torch.empty(1, dtype=torch.int32, pin_memory=True)
        self.count_ready = torch.cuda.Event()
        self.written = torch.cuda.Event()
        self.spec = False
        self.index = 0
        self.M = None                # sample count once the host has read it
        self.loss = torch.empty(1, dtype=torch.float32, device=dev)
        self.samples = None          # [cap_m, 8] fp32: xyzs | dirs | ts (speculative write pass)
        self.cap_m = 0
        self.N = 0
        self.args = None
        self.bits = None             # the occupancy bit field the batch was marched through (keeps its memory alive for `args`)
        self.refreshed = False
        self.pre = None              # what the pipeline held in front of this batch's draw (BatchPipeline.state_dict)


class BatchPipeline:
    """Prepared batches of one engine, which owns it as `engine.batches`.

    In: the cameras (`poses`, `cam_near_far`), the fp32 `images` or the `capture`'s uint8 bank, the model's occupancy bit field, and the
    engine's `num_rays` / `last_num_points` (adaptive ray count: batch j takes N from batch j-1's sample count and writes `num_rays` back).
    Out: a prepared batch (_RayBufs: rays, ground truth, march records, the sample count on its way to the host) -- take() hands the oldest
    one to the step, finish() completes its samples.  Everything is read from the engine when it is used (`overlap`, `depth`, `num_rays`,
    `images` and `_refresh` may be replaced on the instance after construction); no parameter is touched here."""

    def __init__(self, engine, seed, min_rays, single_pass):
        self.eng, self.device = engine, engine.device
        # ONE draw per batch for everything random about it (synthetic.batch_from_uniforms): which batch a number goes to then does not
        # depend on how far ahead batches are prepared, so this executor and Stage0Trainer consume identical draws (rank r: its own rays)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed)
        self.side = L.side_stream(self.device, slot=2)
        self.single_pass = single_pass
        self._min_rays = min_rays
        self._bufs = [None, None, None]
        self._cur = 0
        self._marker = None                   # go-ahead of the side stream: the running step's event (go_ahead)
        self._post_refresh = None             # event behind the batch a refresh forced onto the main stream
        self._mid_fill = False                # a batch is waiting for mid_step_fill()
        self._last = None                     # the newest prepared batch
        self._queue = []                      # prepared batches, oldest first (steady state: the next one and the one after)
        self._prepared = 0                    # index (1-based) of the newest prepared batch
        self._refreshed = 0                   # index of the newest batch whose occupancy refresh has run (a loaded state may be behind its refresh)

    def go_ahead(self, event):
        """The step's marker: the side stream may start the next batch behind `event` (the last kernel that reads the oldest buffer set)."""
        self._marker = event

    def take(self):
        """The batch of the step that starts now."""
        if not self._queue:
            self.fill()
        return self._queue.pop(0)

    # ------------------------------------------------------------------------------------------------------ buffers
    def _ray_bufs(self, N):
        self._cur = (self._cur + 1) % len(self._bufs)
        b = self._bufs[self._cur]
        if b is None or b.cap < N:
            b = self._bufs[self._cur] = _RayBufs(max(int(N * 1.5), self._min_rays), self.device)
        return b

    def _sample_bufs(self, b, cap_m):
        if b.samples is None or b.cap_m < cap_m:
            b.cap_m = int(cap_m)
            b.samples = torch.empty(b.cap_m * 8, dtype=torch.float32, device=self.device)
        c = b.cap_m
        s = b.samples
        return s[:3 * c], s[3 * c:6 * c], s[6 * c:]

    # ------------------------------------------------------------------------------------------------- next batch
    def prepare(self, N, depth_view=None):
        """Batch of N rays (depth_view: a depth batch, its N rays go through the keypoints of that view -- n2m_batch_rays in keypoint mode): pixel choice, rays + ground truth, near/far, march pass 1 (count + offset scan), count on its way to the host.
        Reads the cameras, the images and the occupancy bit field only."""
        eng = self.eng
        opt, model, dev = eng.opt, eng.model, self.device
        cap = eng.capture
        if cap is None and eng.images is None:
            eng.images = synthetic.preload_images(eng.poses, eng.boxes)
        b = self._ray_bufs(N)
        b.N, b.M = N, None
        s = L.stream()
        # one draw for everything random about the batch + one kernel for pixels, rays, ground truth, near/far, jitter, background
        b.u = torch.rand(N, 6, device=dev, generator=self.gen)
        aabb = model.aabb_train
        b.bg = b.bg_buf if opt.background != "white" else None
        b.depth_view = depth_view
        out = (b.o, b.d, b.rgba, b.nears, b.fars, b.noises, b.bg)
        common = dict(counter=b.counter, cam_near_far=eng.cam_near_far)
        if depth_view is not None:
            C.batch_sparse_u8(eng.poses, cap.bank, cap.lut, b.u, depth_view, cap.sparse_depth, aabb, model.min_near, cap.H, cap.W,
                              cap.intrinsics_of(depth_view),       # one view per batch: its four scalars from the host copy (per-view sets too)
                              out=out + (b.gtd, b.dw), **common)
        elif cap is not None:
            dense = eng.dense_depth
            C.batch_from_uniforms_u8(eng.poses, cap.bank, cap.lut, b.u, aabb, model.min_near, cap.H, cap.W, cap.intrinsics,
                                     out=out if dense is None else out + (b.gtd,), dense_depth=dense, **common)
        else:
            synthetic.batch_from_uniforms(eng.poses, eng.images, b.u, aabb, model.min_near, out=out, **common)
        if eng.ind_dim > 0:
            # which view every ray reads: the same uniforms through the batch kernels' own expression (n2m_batch_views); launched only here
            if b.views is None or b.views.numel() < b.cap:
                b.views = torch.empty(b.cap, dtype=torch.int32, device=dev)
            if depth_view is not None:
                b.views[:N].fill_(int(depth_view))
            else:
                C.batch_views(b.u, eng.poses.shape[0], out=b.views)
        bits = model.density_bitfield
        b.args = (_p(b.o), _p(b.d), _p(bits), float(model.real_bound), int(bool(opt.contract)), float(opt.dt_gamma), int(opt.max_steps), N,
                  int(model.cascade), int(model.grid_size), _p(b.nears), _p(b.fars))
        b.bits = bits
        b.spec = b.one_pass = False
        expect = 0 if eng.last_num_points <= 0 else ((int(1.25 * max(eng.last_num_points, 1024)) + 1023) // 1024) * 1024
        if expect > 0 and self.single_pass:
            # march ONCE: count + recorded chunks, then replayed into buffers a quarter above the last batch; a ray that does
            # not fit is skipped like raymarching.cu:417 and finish() then writes the batch exactly from the (offset, count) it left
            x, d, t = self._sample_bufs(b, expect)
            L.call("n2m_march_rays_train_fused", *b.args, _p(x), _p(d), _p(t), _p(b.rays), _p(b.counter), _p(b.noises), b.cap_m,
                   _p(b.ws), b.ws.numel(), s)
            b.host_count.copy_(b.counter, non_blocking=True)
            b.count_ready.record()
            b.spec = b.one_pass = True
            return b
        L.call("n2m_march_rays_train", *b.args, None, None, None, _p(b.rays), _p(b.counter), _p(b.noises), s)
        b.host_count.copy_(b.counter, non_blocking=True)
        b.count_ready.record()
        # speculative pass 2 right behind it, into buffers a quarter above the last batch (adaptive num_rays steers M towards
        # opt.num_points): a ray that does not fit is skipped like raymarching.cu:417 and finish() re-marches the batch exactly.  With
        # batches prepared two ahead the pass has finished a whole step before its samples are read, so the consumer normally needs no
        # cross-stream wait at all (an event that has already fired is not waited for)
        if expect > 0:
            x, d, t = self._sample_bufs(b, expect)
            L.call("n2m_march_rays_train_write", *b.args, _p(x), _p(d), _p(t), _p(b.rays), _p(b.noises), b.cap_m, s)
            b.spec = True
            b.written.record()
        return b

    def count(self, b):
        """Sample count of batch b on the host (waits for the event behind its offset scan; normally long complete; polled, because after
        an occupancy refresh the step cannot be enqueued before this count is known)."""
        if b.M is None:
            L.wait_polled(b.count_ready)
            b.M = int(b.host_count[0])
        return b.M

    def fill(self, max_new=None):
        """Prepare batches until `depth` of them wait in the queue (at most max_new of them in this call).  Batch j takes its ray count from batch j-1's sample count
        (adaptive num_rays, nerf/utils.py:796-797) and, when (j-1) % 16 == 0, follows an occupancy refresh that needs step j-1's
        parameter update: such a batch cannot be prepared early -- it is issued on the main stream behind that step.  Every other batch
        is issued on the side stream behind the marker in front of the running step's Adam kernel: its count pass then runs beside
        the optimizer update (a streaming kernel that leaves the ALUs idle) instead of beside the forward lookup, and its count is on
        the host a whole step before it is needed."""
        eng = self.eng
        opt = eng.opt
        new = 0
        while len(self._queue) < eng.depth and (max_new is None or new < max_new):
            new += 1
            j = self._prepared + 1
            need_refresh = (j - 1) % opt.update_extra_interval == 0
            if need_refresh and j - 1 > eng.global_step:
                break                                   # its refresh waits for a step that is not queued yet
            prev = self._last                           # batch j-1 (still queued, or the one the running step consumes)
            if prev is not None:                        # N(j) from M(j-1)
                M = self.count(prev)
                if opt.adaptive_num_rays and M > 0 and prev.depth_view is None:      # (a depth batch does not steer the ray count)
                    eng.num_rays = max(1, int(round((opt.num_points / M) * prev.N)))
            N = int(eng.num_rays)
            # (what a checkpoint taken while this batch waits in the queue needs: the state in front of its draws, as plain host values)
            pre = (self.gen.get_offset(), N, eng.last_num_points, len(eng.depth_schedule.log) if eng.depth_schedule is not None else None)
            view = eng.depth_schedule.next() if eng.depth_schedule is not None else None
            if view is not None:
                N = eng.capture.sparse_depth.counts[view]
            defer = False
            if need_refresh or not eng.overlap or self._marker is None:
                if need_refresh and self._refreshed < j:
                    eng._refresh()
                    self._refreshed = j
                b = self.prepare(N, view)
                if need_refresh and eng.overlap and self._marker is not None:
                    # the batch behind this one needs THIS batch's count, which the host can only wait for -- and the running step cannot be
                    # enqueued before it has that count either.  So the next batch is prepared right behind the step's first launch (the
                    # lookup: mid_step_fill), on the side stream behind this event instead of the step's marker: it marches beside the
                    # lookup and the field kernels as before, but the GPU no longer idles ~100 us while the host prepares it
                    self._post_refresh = torch.cuda.Event()
                    self._post_refresh.record()
                    self._mid_fill = True
                    defer = True
            else:
                after_refresh = (j - 2) % opt.update_extra_interval == 0 and self._post_refresh is not None
                self.side.wait_event(self._post_refresh if after_refresh else self._marker)
                with torch.cuda.stream(self.side):
                    b = self.prepare(N, view)
                main = torch.cuda.current_stream(self.device)
                b.u.record_stream(main)
            b.index = j
            b.pre = pre
            self._prepared = j
            self._last = b
            self._queue.append(b)
            if defer:
                break

    # ------------------------------------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """The pipeline at a step boundary, as the NEXT batch's preparation met it: the generator in front of that batch's draw, the ray
        count and sample count it saw, the depth schedule's position, and whether its occupancy refresh has run.  The prepared batches
        themselves are not saved: loading prepares them again from the same draws."""
        eng = self.eng
        nxt = self._queue[0].pre if self._queue else None
        gen = self.gen.get_state()
        if nxt is not None:
            g = torch.Generator(device=self.device)
            g.set_state(gen)
            g.set_offset(nxt[0])
            gen = g.get_state()
        _, num_rays, last, pos = nxt if nxt is not None else (None, int(eng.num_rays), eng.last_num_points,
                                                              len(eng.depth_schedule.log) if eng.depth_schedule is not None else None)
        step = self._queue[0].index - 1 if self._queue else self._prepared
        return {"gen": gen, "num_rays": int(num_rays), "last_num_points": int(last), "prepared": int(step),
                "refreshed": int(self._refreshed) if self._refreshed > step else 0,
                "depth_schedule": None if eng.depth_schedule is None else eng.depth_schedule.state_dict(pos)}

    def load_state_dict(self, sd):
        """Drops every prepared batch; the next take() prepares batch `prepared` + 1 from the loaded generator."""
        eng = self.eng
        torch.cuda.current_stream(self.device).wait_stream(self.side)      # (nothing of the dropped batches is still being written)
        self._queue, self._last, self._marker, self._post_refresh, self._mid_fill = [], None, None, None, False
        self._prepared, self._refreshed = int(sd["prepared"]), int(sd.get("refreshed", 0))
        self.gen.set_state(sd["gen"].cpu())
        eng.num_rays, eng.last_num_points = int(sd["num_rays"]), int(sd["last_num_points"])
        if (eng.depth_schedule is None) != (sd.get("depth_schedule") is None):
            raise ValueError("depth_schedule: the checkpoint and this driver disagree on enable_sparse_depth")
        if eng.depth_schedule is not None:
            eng.depth_schedule.load_state_dict(sd["depth_schedule"])

    def mid_step_fill(self):
        """Behind the step's first launch: the one batch whose preparation the refresh in front of this step had to put off."""
        if self._mid_fill:
            self._mid_fill = False
            self.fill(max_new=1)

    def finish(self, b):
        """Samples of batch b: the speculative pass 2 of prepare() when the count fits its buffers (the normal case), else an exact
        pass 2 on the main stream (the host has waited for the event behind the offset scan, so no cross-stream dependency is needed)."""
        M = self.count(b)
        if M > 0 and b.spec and M <= b.cap_m:
            if not b.one_pass and not b.written.query():      # (single pass: the host has seen the count, which the same kernel wrote last)
                torch.cuda.current_stream(self.device).wait_event(b.written)
        elif M > 0:
            x, d, t = self._sample_bufs(b, ((int(1.25 * M) + 1023) // 1024) * 1024 if b.cap_m < M else b.cap_m)
            L.call("n2m_march_rays_train_write", *b.args, _p(x), _p(d), _p(t), _p(b.rays), _p(b.noises), b.cap_m, L.stream())
        return M
