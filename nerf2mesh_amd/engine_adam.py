"""The optimizer pass of the stage-0 step executor (engine.Stage0Engine): the N2mAdamDesc descriptors of its three forms (whole tensors, level
halves, the rank's own shard), the double-buffered table state of the fused pass, the sharded layout with its row gathers, and the launch
sequence n2m_adam_step[_peer | _scaler] -> [n2m_adam_fuse_restore] -> [row exchange] -> n2m_scaler_update_slots -> learning rate."""
import ctypes

import torch

from . import _lib as L

_p = L.ptr


def lr_lambda(it, iters):
    """main.py:239: 0.01 -> 1 over the first 500 iterations, then 0.1 ** ((it - 500) / (iters - 500))."""
    return 0.01 + 0.99 * (it / 500) if it <= 500 else 0.1 ** ((it - 500) / (iters - 500))


def peer_chunk_rows(split, world, pad=0):
    """Rows of one rank's chunk of the coarse half [0, split) in peer-store mode: split / world rounded UP to a multiple of four (+ pad), so that
    every chunk starts 16-byte aligned in the packed table (8-byte rows, stored as 16-byte row pairs) and holds a multiple of four rows; the last
    rank's chunk is what is left.  None when the layout does not exist (split not a multiple of four, or the padding leaves the last rank empty)."""
    if split % 4 != 0 or pad % 4 != 0:
        return None
    cs = (split + 4 * world - 1) // (4 * world) * 4 + pad
    return cs if (world - 1) * cs < split else None


class ShardLayout:
    """Rows of the two tables by owner: the coarse half [0, split) (levels 0..7) in chunks of `rows_c` (padded chunks: the last rank's is
    shorter, `uneven`), the fine half [split, rows) (levels 8..15) in chunks of `rows_f`."""

    def __init__(self, rank, world, split, rows_c, rows_f, uneven=False):
        self.rank, self.world, self.split, self.rows_c, self.rows_f, self.uneven = rank, world, split, rows_c, rows_f, uneven

    def ranges_of(self, r):
        c0 = min(self.split, r * self.rows_c)
        return {"c": (c0, min(self.rows_c, self.split - c0)), "f": (self.split + r * self.rows_f, self.rows_f)}

    def ranges(self):
        """(first row, rows) of this rank's slice of the coarse half and of the fine half."""
        return self.ranges_of(self.rank)

    def first_row(self, h):
        return 0 if h == "c" else self.split


def fill_entry(desc, k, param, state, grad, slot, *, row0=0, rows=None, cols=1, grad_bytes=0, shadow=None, shadow_mode=0, grad_is_half=0,
               clear_grad=0):
    """Entry k of an N2mAdamDesc: `rows` rows of `cols` columns from row `row0` of `param` and its moments (None: the whole tensor);
    `grad` from the same row on when `grad_bytes` (bytes per gradient element) is given, else from its start; `shadow`: the packed table,
    whose same rows the pass refreshes (shadow_mode 2: the density column, 3: the colour columns)."""
    off = row0 * cols * 4
    desc.param[k], desc.grad[k] = param.data_ptr() + off, grad.data_ptr() + row0 * cols * grad_bytes
    desc.exp_avg[k], desc.exp_avg_sq[k] = state["exp_avg"].data_ptr() + off, state["exp_avg_sq"].data_ptr() + off
    desc.half_shadow[k] = None if shadow is None else shadow.data_ptr() + row0 * 8
    desc.shadow_mode[k] = shadow_mode
    desc.numel[k] = param.numel() if rows is None else rows * cols
    desc.grad_is_half[k], desc.clear_grad[k], desc.slot[k] = grad_is_half, clear_grad, slot


class AdamPass:
    """What Stage0Engine owns as `engine.adam`.  Reads the engine's model, optimizer, gradient buffers, shard layout and peer exchange."""

    def __init__(self, engine):
        self.eng = engine
        self._desc = {}
        self.packed = None           # the packed table the newest descriptor names
        self.gathers = {}            # row gathers of the last sharded pass that nobody has waited for yet, by level half
        self.fine_ready = None       # lookup_overlap: event behind the fine half of the last pass
        self._synced = (-1, False, False)
        self._adam_peer = None

    def reset(self):
        """Behind a loaded checkpoint: the optimizer's moment tensors were replaced (FusedAdamAMP.state_epoch already keys the descriptors on
        that) -- drop every cached descriptor anyway, the lookup-overlap event of a pass that no longer counts, and the fused pass's other
        buffer set, which holds the values of a step before the load."""
        self.wait_gather()
        self._desc, self.packed, self.fine_ready, self._synced = {}, None, None, (-1, False, False)
        if self.eng.fuse_adam is not None:
            self.eng.fuse_adam.update(alt=None, desc={})

    # ------------------------------------------------------------------------------------------------ descriptors
    def _tables(self, pk, g1, g2, row0=0, rows=None, whole_grads=False):
        """Entries of the two tables, `rows` rows from `row0` (None: all).  whole_grads: g1 / g2 are the full gradient buffers, read from
        the same row on (fp32 and fp16 elements); else they are slices that start at the entry's first row."""
        model = self.eng.model
        return [(model.encoder.embeddings, g1, dict(row0=row0, rows=rows, cols=1, shadow=pk, shadow_mode=2, grad_bytes=4 if whole_grads else 0)),
                (model.encoder_color.embeddings, g2, dict(row0=row0, rows=rows, cols=2, shadow=pk, shadow_mode=3, grad_is_half=1,
                                                          grad_bytes=2 if whole_grads else 0))]

    def _mlp(self, full):
        """Entries of the MLP weights in the optimizer's order (`full`: the specular head takes part)."""
        eng = self.eng
        live = dict(zip(eng.mlp_params[:7 if full else 5], eng.dw_views))
        return [(p, live[p], dict(clear_grad=1)) for g in eng.optimizer.param_groups for p in g["params"] if p in live]

    def _build(self, entries):
        """(descriptor, participants mask, param group of every entry) from (param, grad, fill_entry keywords) entries."""
        o = self.eng.optimizer
        group_of = {p: gi for gi, g in enumerate(o.param_groups) for p in g["params"]}
        desc, participants, groups = L.AdamDesc(), 0, []
        for k, (p, g, kw) in enumerate(entries):
            fill_entry(desc, k, p, o.state[p], g, o._slot[p], **kw)
            participants |= 1 << (o._slot[p] - 1)
            groups.append(group_of[p])
        desc.count = len(entries)
        return desc, participants, groups

    def _set_lr(self, desc, groups, lr_factor):
        o = self.eng.optimizer
        for k, gi in enumerate(groups):
            desc.lr[k] = float(o.param_groups[gi]["initial_lr"]) * lr_factor

    def desc(self, full, dense_only=False):
        """The N2mAdamDesc of this model (pointers are fixed for the life of the engine); `full`: the specular head takes part;
        `dense_only`: the two tables take part with their rows below fuse_adam['first_row'] only (the others got their update inside the
        table backward)."""
        eng = self.eng
        o, model = eng.optimizer, eng.model
        # packed_tables() hands out a NEW tensor whenever a table was changed through torch (load_state_dict, an in-place edit): the
        # descriptor carries its address (Adam refreshes the copy the forward gathers from), so the address is part of the key
        pk = model.packed_tables()
        assert pk is not None
        if eng.peer is not None and pk.data_ptr() != eng.peer.packed.data_ptr():
            raise RuntimeError("peer-store exchange: the packed table left the exported buffer (peers would keep writing into the old one)")
        key = (full, getattr(o, "state_epoch", 0), pk.data_ptr(), model.encoder.embeddings.data_ptr(), model.encoder_color.embeddings.data_ptr(),
               dense_only)
        d = self._desc.get(key)
        if d is not None:
            return d
        live = lambda k: k[1:3] == key[1:3] and (k[3:5] == key[3:5] or (eng.fuse_adam is not None and self.is_alt(k[3], k[4])))
        self._desc = {k: v for k, v in self._desc.items() if live(k)}      # drop descriptors of an older table / state generation
        self.packed = pk
        if eng.shard:
            # the rank's OWN rows: per level half one [rows,1] + one [rows,2] entry (pointers offset into the full state tensors, gradients =
            # the reduce-scattered slices, working copy = the same rows of the packed table), then the MLP weights
            entries = [e for h, (row0, n) in eng.layout.ranges().items() for e in self._tables(pk, eng.g1s[h], eng.g2s[h], row0=row0, rows=n)]
            entries += self._mlp(full)
        else:
            entries = self._tables(pk, eng.g1, eng.g2, rows=eng.fuse_adam["first_row"] if dense_only else None) + self._mlp(full)
            if eng.ind_dim > 0:      # lr x 0.1, no weight decay (renderer.get_params); same found_inf skip as every other tensor of the pass
                entries.append((model.individual_codes, eng.dcodes, dict(clear_grad=1)))
            if eng.opt.sdf:          # the NeuS variance (lr x 0.1, nerf/network.py:186): its gradient is a scalar the SDF head's backward leaves in d_var
                entries.append((model.variance, eng._sdf_buf()["d_var"], {}))
            order = {p: i for i, p in enumerate(p for g in o.param_groups for p in g["params"])}
            entries.sort(key=lambda e: order[e[0]])      # the optimizer's order
        d = self._desc[key] = self._build(entries)
        return d

    def desc_halves(self, full, lr_factor):
        """(fine, coarse) descriptors of the single-GPU optimizer pass in two calls: rows [ho[8], rows) of both tables | rows [0, ho[8]) of both
        tables + the MLP weights.  Pointers are offsets into the same tensors n2m_adam_step takes in one call (desc)."""
        eng = self.eng
        o, model = eng.optimizer, eng.model
        pk = model.packed_tables()
        key = ("halves", full, getattr(o, "state_epoch", 0), pk.data_ptr(), model.encoder.embeddings.data_ptr(), model.encoder_color.embeddings.data_ptr())
        cached = self._desc.get(key)
        if cached is None:
            self.packed = pk
            split = int(eng.ho[8])
            fine = self._tables(pk, eng.g1, eng.g2, row0=split, rows=eng.rows - split, whole_grads=True)
            coarse = self._tables(pk, eng.g1, eng.g2, row0=0, rows=split, whole_grads=True) + self._mlp(full)
            cached = self._desc[key] = (self._build(fine), self._build(coarse))
        for d, _, groups in cached:
            self._set_lr(d, groups, lr_factor)
        return cached[0][0], cached[1][0]

    # ---- double-buffered table state of the fused optimizer pass
    def is_alt(self, p1_ptr, p2_ptr):
        alt = self.eng.fuse_adam["alt"]
        return alt is not None and alt["p"][0].data_ptr() == p1_ptr and alt["p"][1].data_ptr() == p2_ptr

    def fuse_desc(self, lr_factor):
        """N2mAdamFuse for this step: live set = what the model / optimizer name now, other set = fuse_adam['alt']."""
        f, o, model = self.eng.fuse_adam, self.eng.optimizer, self.eng.model
        ps = (model.encoder.embeddings, model.encoder_color.embeddings)
        if f["alt"] is None or getattr(o, "state_epoch", 0) != f.get("epoch"):
            f["alt"] = {"p": [torch.empty_like(p.data) for p in ps], "m": [torch.empty_like(p.data) for p in ps],
                        "v": [torch.empty_like(p.data) for p in ps]}
            f["epoch"], f["desc"] = getattr(o, "state_epoch", 0), {}
        alt = f["alt"]
        key = (ps[0].data_ptr(), ps[1].data_ptr(), self.packed.data_ptr())
        d = f["desc"].get(key)
        if d is None:
            d = L.AdamFuse()
            for t, p in enumerate(ps):
                st = o.state[p]
                d.p_in[t], d.m_in[t], d.v_in[t] = p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                d.p_out[t], d.m_out[t], d.v_out[t] = alt["p"][t].data_ptr(), alt["m"][t].data_ptr(), alt["v"][t].data_ptr()
                d.slot[t] = o._slot[p]
            d.packed, d.first_level = self.packed.data_ptr(), f["first_level"]
            d.beta1, d.beta2 = (float(x) for x in o.param_groups[0]["betas"])
            d.eps, d.scale, d.bias = float(o.param_groups[0]["eps"]), o.scale.data_ptr(), o.bias.data_ptr()
            f["desc"] = {k: v for k, v in f["desc"].items() if k[2] == key[2]}
            f["desc"][key] = d
        group_of = {p: g for g in o.param_groups for p in g["params"]}
        for t, p in enumerate(ps):
            d.lr[t] = float(group_of[p]["initial_lr"]) * lr_factor
        return d

    def _fuse_swap(self):
        """The other buffer set holds the state of the finished step (n2m_adam_fuse_restore has completed it): make it the one the model
        and the optimizer name."""
        alt, o, model = self.eng.fuse_adam["alt"], self.eng.optimizer, self.eng.model
        for t, p in enumerate((model.encoder.embeddings, model.encoder_color.embeddings)):
            st = o.state[p]
            p.data, alt["p"][t] = alt["p"][t], p.data
            st["exp_avg"], alt["m"][t] = alt["m"][t], st["exp_avg"]
            st["exp_avg_sq"], alt["v"][t] = alt["v"][t], st["exp_avg_sq"]
        a, b = model.encoder.embeddings, model.encoder_color.embeddings
        model._packed_key = (a._version, b._version, a.data_ptr(), b.data_ptr())       # same values, new address: the packed copy stays valid

    # ---- sharded pass: the rows every rank has refreshed travel to the others
    def _gather_packed(self):
        """All-gather of the packed rows after the sharded Adam (each rank has refreshed its own rows), as two chunks: the coarse half of the
        levels (32 % of the bytes) first, then the fine half.  Nothing is waited for here: the next step's lookup waits for the coarse chunk,
        looks its eight levels up (n2m_grid_encode_forward_packed_levels) while the fine chunk is still on the wire, then waits for that one
        (wait_gather); everything else that reads the packed table or writes this rank's rows waits for both first."""
        import torch.distributed as dist
        eng, lay = self.eng, self.eng.layout
        flat = self.packed.view(-1)                 # [rows * 2] fp32 words, 8 bytes per row
        self.gathers = {}
        for h, (row0, n) in lay.ranges().items():
            lo = lay.first_row(h)
            out = flat[lo * 2:(lo + lay.world * n) * 2]
            mine = flat[row0 * 2:(row0 + n) * 2]
            self.gathers[h] = dist.all_gather_into_tensor(out, mine if eng._inplace_gather else mine.clone(), async_op=True)
        if not eng.chunked_gather:
            self.wait_gather()

    def wait_gather(self, which=("c", "f")):
        g = self.gathers
        if not g:
            return
        for h in which:
            w = g.pop(h, None)
            if w is not None:
                w.wait()

    def sync_parameters(self, density_only=False, moments=False):
        """Stage0Engine.sync_parameters (its docstring says what for)."""
        eng = self.eng
        if not eng.shard:
            return
        self.wait_gather()
        if eng.peer is not None:
            eng.peer.check()
        # COLLECTIVE: every rank must call it at the same step.  A repeat at the same step is a no-op (so a rank may evaluate or save on
        # its own after all ranks have synchronised once -- bench.py's rank 0 does).  moments=True also gathers Adam's exp_avg / exp_avg_sq
        # of both tables (each rank has only advanced its own rows): what a checkpoint needs -- FusedAdamAMP.state_dict() of a sharded
        # run calls it, so optimizer.state_dict() is a collective too (the reference saves complete optimizer state, nerf/utils.py:1336-1350)
        done = self._synced
        level = (not density_only, moments)
        if done[0] == eng.global_step and (done[1] or density_only) and (done[2] or not moments):
            return
        self._synced = (eng.global_step, level[0] or (done[0] == eng.global_step and done[1]), level[1] or (done[0] == eng.global_step and done[2]))
        import torch.distributed as dist
        lay = eng.layout
        e1p, e2p = eng.model.encoder.embeddings, eng.model.encoder_color.embeddings
        tables = [(e1p.data, 1)] if density_only else [(e1p.data, 1), (e2p.data, 2)]
        if moments:
            for p, C in ((e1p, 1), (e2p, 2)):
                st = eng.optimizer.state[p]
                tables += [(st["exp_avg"], C), (st["exp_avg_sq"], C)]
        for t, C in tables:
            flat = t.view(-1)
            for h, (row0, n) in lay.ranges().items():
                lo = lay.first_row(h)
                if h == "c" and lay.uneven:      # padded chunks (peer-store mode): the last one is shorter -- one broadcast per owner
                    for r in range(lay.world):
                        r0, rn = lay.ranges_of(r)["c"]
                        if rn > 0:
                            dist.broadcast(flat[r0 * C:(r0 + rn) * C], src=r)
                    continue
                dist.all_gather_into_tensor(flat[lo * C:(lo + lay.world * n) * C], flat[row0 * C:(row0 + n) * C].clone())

    # ------------------------------------------------------------------------------------------------------- the pass
    def _scaler_tail(self, participants, loss_out):
        """N2mScalerTail of this step: the scaler / step-count bookkeeping and, with loss_out = (n_rays, loss buffer, (specular partials, scale)
        or None[, (eikonal partials, count, scale)]), the step's loss value from the compositing kernel's per-workgroup partials."""
        eng, o = self.eng, self.eng.optimizer
        gf, bf, gi = o.growth
        tail = L.ScalerTail(growth_tracker=_p(o.growth_tracker), steps=_p(o.steps), participants=participants, growth_factor=gf, backoff_factor=bf,
                            growth_interval=gi, ticket=_p(eng._tail_ticket))
        if loss_out is not None:
            n_rays, buf, extra = loss_out[:3]
            ex_buf, ex_scale = extra if extra is not None else (None, 0.0)
            e2_buf, e2_n, e2_scale = loss_out[3] if len(loss_out) > 3 and loss_out[3] is not None else (None, 0, 0.0)
            tail.loss_partial, tail.n_partial, tail.n_rays, tail.loss, tail.loss_sum = _p(eng._w["partial"]), (n_rays + 15) // 16, n_rays, _p(buf), _p(eng._loss_sum)
            tail.extra_partial, tail.n_extra, tail.extra_scale = _p(ex_buf), eng._n_spec, float(ex_scale)
            tail.extra2_partial, tail.n_extra2, tail.extra2_scale = _p(e2_buf), int(e2_n), float(e2_scale)
        return tail

    def step(self, full, lr_factor, loss_out=None, fused=None):
        eng, o = self.eng, self.eng.optimizer
        self.wait_gather()          # (a step without samples ran no lookup: the rows the last gather sends must not be rewritten under it)
        desc, participants, groups = self.desc(full, dense_only=fused is not None)
        self._set_lr(desc, groups, lr_factor)
        b1, b2 = o.param_groups[0]["betas"]
        adam = (float(b1), float(b2), float(o.param_groups[0]["eps"]), _p(o.scale), _p(o.found_inf), _p(o.bias))
        s = L.stream()
        peer_fused = eng.peer is not None and eng._peer_fused
        scaler_done = False
        if eng.lookup_overlap and fused is None and not eng.shard and eng.Lv == 16:
            # fine rows (levels 8..15) first, an event behind them, then the coarse rows + every other tensor
            d_f, d_c = self.desc_halves(full, lr_factor)
            for d in (d_f, d_c):
                L.call("n2m_adam_step", ctypes.addressof(d), *adam, s)
                if d is d_f:
                    self.fine_ready = torch.cuda.Event()
                    self.fine_ready.record()
        elif peer_fused:
            if self._adam_peer is None:     # entries 0..3 of the sharded descriptor: (density, colour) of the coarse half, then of the fine half
                self._adam_peer = eng.peer.adam_peer([("s1", "c"), ("s2", "c"), ("s1", "f"), ("s2", "f")] + [None] * (desc.count - 4))
            L.call("n2m_adam_step_peer", ctypes.addressof(desc), *adam, ctypes.addressof(self._adam_peer), s)
        elif (eng.adam_tail and loss_out is not None and fused is None and eng.peer is None and not eng.shard):
            # optimizer pass + the scaler / step counts / loss value in one launch (the tail of the pass's last workgroup)
            tail = self._scaler_tail(participants, loss_out)
            L.call("n2m_adam_step_scaler", ctypes.addressof(desc), *adam, ctypes.addressof(tail), s)
            scaler_done = True
        else:
            L.call("n2m_adam_step", ctypes.addressof(desc), *adam, s)
        # (the pass refreshes the packed copy; a plain fp16 copy of the colour table somebody took -- a colour-only call, an export -- is stale now and
        #  no version counter says so: rebuilt on next use, as trainer.Stage0Trainer's shadow callback arranges it)
        eng.model.encoder_color._half_version = -1
        if fused is not None:      # behind both optimizer passes, in front of the scaler update that clears found_inf
            L.call("n2m_adam_fuse_restore", ctypes.addressof(fused), eng.ho.ctypes.data, eng.Lv, _p(o.found_inf), s)
            self._fuse_swap()
        if eng.peer is not None:      # this rank's refreshed rows into every rank's packed table, coarse chunk first; the next lookup waits per half
            for h, (row0, n) in eng.layout.ranges().items():
                if peer_fused:
                    eng.peer.signal_rows(h)               # (Adam has stored them everywhere itself)
                else:
                    eng.peer.push_rows(h, row0, n)
            self.gathers = eng.peer.rows_tokens()
            if not eng.chunked_gather:
                self.wait_gather()
        elif eng.shard:
            self._gather_packed()
        if not scaler_done:        # + the step's loss value from the compositing kernel's per-workgroup partials, when there is one
            tail = self._scaler_tail(participants, loss_out)
            L.call("n2m_scaler_update_slots", _p(o.scale), _p(o.found_inf), _p(o.bias), float(b1), float(b2), ctypes.addressof(tail), s)
        nxt = lr_lambda(eng.global_step, eng.opt.iters)          # like LambdaLR.step(): param_groups carry the NEXT step's rate
        for group in o.param_groups:
            group["lr"] = float(group["initial_lr"]) * nxt
