"""The SDF recipe (config 5) of the stage-0 step executor, as functions of the engine (engine.Stage0Engine._step_sdf / _sdf_buf forward
here): NeuS alpha, finite-difference normals from six offset copies of the batch, eikonal loss, progressive levels."""
import ctypes
import types

import torch

from . import _lib as L

_p = L.ptr


def sdf_buf(eng, M=0):
    """Buffers of the SDF head, grow-only: the six finite-difference copies of the batch (points, [0,1] points, density features, sdf
    values and their gradients), alpha, per-workgroup partials, the variance gradient."""
    if eng._sdf is None or M > eng._sdf_cap:
        cap = max(eng._sdf_cap, int(M * 1.25) + 1024)
        dev = eng.device
        f = lambda n: torch.empty(n, dtype=torch.float32, device=dev)
        old = eng._sdf
        eng._sdf = {"pts": f(18 * cap), "pts01": f(18 * cap), "h6": f(16 * 6 * cap), "d_h6": f(16 * 6 * cap), "s6": f(6 * cap), "d_s6": f(6 * cap),
                    "alpha": f(cap), "d_sdf": f(cap), "x01": f(3 * cap), "eik": f((cap + 255) // 256 + 1), "varp": f((cap + 255) // 256 + 1),
                    "d_var": old["d_var"] if old is not None else torch.zeros(1, dtype=torch.float32, device=dev),      # (the Adam descriptor holds its address)
                    # folded copies (n2m_sdf_fold_*): per-sample flags, the compact list of the copies that keep the stacked pass
                    "fold_cnt": old["fold_cnt"] if old is not None else torch.zeros(2, 32, dtype=torch.int32, device=dev),
                    "fold_host": old["fold_host"] if old is not None else torch.zeros(32, dtype=torch.int32).pin_memory()}
        eng._sdf_cap = cap
    return eng._sdf


def step_sdf(eng, st):
    """The iteration of the SDF recipe (nerf/renderer.py:724-741, nerf/network.py:143-154, nerf/utils.py:651-655,740-743) as a fixed launch
    sequence: lookup -> field (raw sdf) -> six finite-difference copies through the density encoder + sigma_net (ONE stacked call each
    way) -> NeuS alpha (n2m_sdf_alpha_forward) -> compositing + loss in alpha mode -> n2m_sdf_alpha_backward (+ eikonal) -> field
    backward (batch and stacked copies) -> table backward (shared fill for the batch, the density table alone for the copies, TV) ->
    Adam (+ the variance) -> bookkeeping (loss = photometric + specular + eikonal terms).  trainer.Stage0Trainer is the parity baseline.
    st: the step's shared values (engine._Step)."""
    opt, M = eng.opt, st.M
    q = types.SimpleNamespace(sb=sdf_buf(eng, M), ml=int(min(eng.model.max_level, eng.Lv)), eps=float(opt.normal_anneal_epsilon),
                              car=float(opt.cos_anneal_ratio), fold=False)
    extra = extra2 = None
    if M > 0:
        _forward_chain(eng, st, q)
    _head(eng, st, q)
    if M > 0:
        lam_eik = _backward_chain(eng, st, q)
        _table_backward(eng, st, q)
        if st.spec_reg:
            extra = (st.w["spec_partial"], float(opt.lambda_specular / M))
        if lam_eik > 0:
            extra2 = (q.sb["eik"], (M + 255) // 256, float(lam_eik / M))
    else:
        eng.g1.zero_()
        eng.g2.zero_()
        q.sb["d_var"].zero_()
    eng._go_ahead()
    eng._lr_step(st.shading != 0, loss_out=(st.N, st.b.loss, extra, extra2))
    loss = st.b.loss.view(())
    eng._fill_pipeline()
    return loss


def _forward_chain(eng, st, q):
    """Lookup, field (raw sdf), the six offset copies through the density encoder + sigma_net, NeuS alpha; plans the fold on the way."""
    opt, model, dev = eng.opt, eng.model, eng.device
    w, sb, M, ml, s = st.w, q.sb, st.M, q.ml, st.s
    e1 = model.encoder
    M6 = 6 * M
    if ml < eng.Lv:          # progressive levels: the kernels leave the inactive levels alone, the field reads all sixteen
        w["h1"][ml * M:16 * M].zero_()
        w["h2"][2 * ml * M:32 * M].zero_()
        sb["h6"][ml * M6:16 * M6].zero_()
    eng.adam.wait_gather()
    L.call("n2m_grid_encode_forward_packed", _p(st.xyzs), _p(st.pk), _p(e1.offsets), _p(w["h1"]), _p(w["h2"]), M, eng.Lv, ml, eng.S,
           eng.H0, *st.geo, *st.aff, s)
    eng._mid_step_fill()
    L.call("n2m_field_forward_train", _p(st.xyzs), st.dirs_p, _p(w["h1"]), _p(w["h2"]), *st.wp, M, st.shading, 3,
           _p(w["sigma"]), _p(w["rgb"]), None, _p(w["spec_partial"]) if st.spec_reg else None, s)
    # finite-difference normals: six offset copies, one encode + one sigma_net evaluation for all of them
    L.call("n2m_sdf_offsets", _p(st.xyzs), M, q.eps, float(model.bound), _p(sb["pts"]), _p(sb["pts01"]), s)
    # Table backward of the copies: once epsilon is a fraction of the finest active cell, a copy nearly always lies in its centre
    # sample's cell on a given level -- those (copy, level) pairs fold into the batch's own backward
    # (n2m_grid_encode_backward_binned_pair_fold), the others (2.4 % at the end of the schedule) take a density-only call over
    # per-level lists whose lengths the host reads back (known long before the backward is enqueued: the plan only needs the samples)
    finest = eng.H0 * 2.0 ** (eng.S * (ml - 1))
    # (the fold and the lists call are one-pass paths of the table backward: batches above 2^20 samples keep the stacked pass)
    q.fold = eng.sdf_fold and q.eps / (2.0 * float(model.bound)) * finest < 0.25 and M <= (1 << 20)
    if q.fold:
        if "fold" not in sb:      # buffers of the fold, only once it is used: per-level flags and lists (capacity: every copy)
            c6 = 6 * eng._sdf_cap
            sb["fold"] = {"cap": c6, "flags": torch.empty(16 * eng._sdf_cap, dtype=torch.uint8, device=dev),
                          "pts": torch.empty(16 * c6 * 3, dtype=torch.float32, device=dev),
                          "src": torch.empty(16 * c6, dtype=torch.int32, device=dev), "g": torch.empty(16 * c6, dtype=torch.float32, device=dev)}
        fb = sb["fold"]
        q.par = eng.global_step & 1
        # the plan kernel adds onto this parity's counters and clears the other parity's for the next step -- which only holds while
        # every step runs the plan; a step without it (no samples, the fold condition off for a step) would leave counts behind
        sb["fold_cnt"][q.par].zero_()
        L.call("n2m_sdf_fold_plan", _p(st.xyzs), M, q.eps, float(model.bound), eng.Lv, ml, eng.S, eng.H0, st.geo[1],
               _p(fb["flags"]), _p(fb["pts"]), _p(fb["src"]), fb["cap"], _p(sb["fold_cnt"]), q.par, s)
        sb["fold_host"].copy_(sb["fold_cnt"][q.par], non_blocking=True)
        q.fold_ready = torch.cuda.Event()
        q.fold_ready.record()
    L.call("n2m_grid_encode_forward", _p(sb["pts01"]), _p(e1.embeddings), _p(e1.offsets), _p(sb["h6"]), M6, 3, 1, eng.Lv, ml, eng.S, eng.H0,
           None, *st.geo, L.F32, s)
    L.call("n2m_field_forward", _p(sb["pts"]), None, _p(sb["h6"]), None, *st.wp, M6, 0, 2, _p(sb["s6"]), None, None, s)
    L.call("n2m_sdf_alpha_forward", _p(w["sigma"]), _p(sb["s6"]), _p(st.dirs), _p(st.ts), M, _p(model.variance), q.eps, q.car, _p(sb["alpha"]), None,
           _p(sb["eik"]) if opt.lambda_eikonal > 0 else None, s)


def _head(eng, st, q):
    """Compositing in alpha mode + loss head + their backward."""
    opt, w, b = eng.opt, st.w, st.b
    bg_t, bg_s = (b.bg, 0.0) if b.bg is not None else (None, 1.0)
    head = L.CompositeLoss(sigmas=_p(q.sb["alpha"]), rgbs=_p(w["rgb"]), ts=_p(st.ts), rays=_p(b.rays), M=st.M, N=st.N, T_thresh=1e-4,
                           gt_rgba=_p(b.rgba), bg=_p(bg_t), bg_scalar=bg_s, lambda_rgb=float(opt.lambda_rgb), lambda_mask=eng._lambda_mask(),
                           grad_loss=_p(st.seed), grad_sigmas=_p(st.d_sigma), grad_rgbs=_p(st.d_rgb), partial=_p(w["partial"]), alpha_mode=1)
    L.call("n2m_composite_loss_train", ctypes.addressof(head), st.s)


def _backward_chain(eng, st, q):
    """NeuS alpha backward (+ eikonal), field backward of the batch and of the stacked copies.  Returns the eikonal weight."""
    opt, model, o = eng.opt, eng.model, eng.optimizer
    w, sb, M, s = st.w, q.sb, st.M, st.s
    lam_eik = float(opt.lambda_eikonal) if opt.lambda_eikonal > 0 else 0.0
    L.call("n2m_sdf_alpha_backward", _p(st.d_sigma), _p(w["sigma"]), _p(sb["s6"]), _p(st.dirs), _p(st.ts), M, _p(model.variance), q.eps, q.car,
           _p(st.seed), float(lam_eik * 2.0 / M), _p(sb["d_sdf"]), _p(sb["d_s6"]), _p(sb["varp"]), _p(sb["d_var"]), _p(o.found_inf), s)
    L.call("n2m_field_backward_train", _p(st.xyzs), st.dirs_p, _p(w["h1"]), _p(w["h2"]), *st.wp, M, st.shading, 3,
           _p(sb["d_sdf"]), _p(st.d_rgb), None, _p(w["d_h1"]), _p(w["d_h2"]), *eng._dw_ptrs, _p(o.found_inf),
           float(2.0 * opt.lambda_specular / M) if st.spec_reg else 0.0, _p(st.seed) if st.spec_reg else None, s)
    L.call("n2m_field_backward", _p(sb["pts"]), None, _p(sb["h6"]), None, *st.wp, 6 * M, 0, 2, _p(sb["d_s6"]), None, None,
           _p(sb["d_h6"]), None, *eng._dw_ptrs, _p(o.found_inf), s)
    return lam_eik


def _fold_decision(q):
    """The host reads the per-level counts of the copies the fold leaves over (polled: the plan ran long ago).  Returns the longest
    level's count and the total."""
    L.wait_polled(q.fold_ready)
    return int(q.sb["fold_host"][:q.ml].max()), int(q.sb["fold_host"][:q.ml].sum())


def _table_backward(eng, st, q):
    """Table gradients: the batch through the shared fill (both tables, overwrite), the stacked copies onto the density table alone --
    folded into the batch's call where the plan allows it -- and the TV term."""
    opt, model, dev, o = eng.opt, eng.model, eng.device, eng.optimizer
    w, sb, M, ml, s = st.w, q.sb, st.M, q.ml, st.s
    e1 = model.encoder
    M6 = 6 * M
    ho = eng.ho.ctypes.data
    L.grid_backward_config(*eng._bwd_cfg)
    need = max(L.lib().n2m_grid_binned_pair_workspace_bytes(M, ml, ho), L.lib().n2m_grid_binned_pair_workspace_bytes(M6, ml, ho))
    ws = L.workspace(dev, need)
    tv_fold = opt.lambda_tv > 0 and ml == eng.Lv
    geo = (eng.Lv, ml, eng.S, eng.H0, *st.geo)
    geo_batch = geo
    if opt.lambda_tv > 0 and 6 <= ml < eng.Lv and eng.sdf_tv_all:
        # progressive levels: the TV term covers ALL sixteen levels (grid.py:170-192 has no max_level).  Instead of the batch's backward
        # over the active levels + the TV as its own 16-level pass (185 us), the batch's backward runs over all sixteen with the TV
        # folded in and ZERO feature gradients on the inactive levels (the encoder's backward ignores them, grid.py:71-95): one pass
        # on the 1-D XCD grid.  Pays from about six active levels on.
        w["d_h1"][ml * M:16 * M].zero_()
        w["d_h2"][2 * ml * M:32 * M].zero_()
        geo_batch = (eng.Lv, eng.Lv) + geo[2:]
        tv_fold = True
        ws = L.workspace(dev, max(need, L.lib().n2m_grid_binned_pair_workspace_bytes(M, eng.Lv, ho)))
    batch_args = (_p(w["d_h1"]), _p(w["d_h2"]), _p(st.xyzs), ho, _p(eng.g1), _p(eng.g2), M, *geo_batch,
                  _p(e1.embeddings) if tv_fold else None, *st.tv, _p(st.seed) if tv_fold else None, _p(o.found_inf),
                  *st.aff, 1, _p(ws), ws.numel())
    fold = q.fold
    if fold:
        K, eng.last_fold_left = _fold_decision(q)
        if K > (1 << 20):      # a level's list of unfolded copies exceeds the one-pass limit of the lists call: this step keeps the stacked pass
            fold = False
    if fold:
        fb = sb["fold"]
        L.call("n2m_grid_encode_backward_binned_pair_fold", *batch_args, _p(fb["flags"]), _p(sb["d_h6"]), q.eps, float(model.bound), s)
        if K > 0:
            L.call("n2m_sdf_fold_gather", _p(sb["d_h6"]), M, ml, _p(fb["src"]), _p(fb["pts"]), fb["cap"],
                   sb["fold_cnt"].data_ptr() + 128 * q.par, K, _p(fb["g"]), s)
            L.call("n2m_grid_encode_backward_binned_lists", _p(fb["g"]), _p(fb["pts"]), fb["cap"], ho, _p(eng.g1), K, *geo,
                   _p(o.found_inf), 0, _p(ws), ws.numel(), s)
    else:
        L.call("n2m_grid_encode_backward_binned_pair", *batch_args, s)
        L.call("n2m_grid_encode_backward_binned_pair", _p(sb["d_h6"]), None, _p(sb["pts01"]), ho, _p(eng.g1), None, M6, *geo,
               None, 0.0, 0.0, 1.0, None, _p(o.found_inf), 1.0, 0.0, 0, _p(ws), ws.numel(), s)
    if opt.lambda_tv > 0 and not tv_fold:
        # progressive levels: the TV term covers ALL levels of the table (grid.py:170-192 has no max_level), as its own pass
        x01 = sb["x01"][:3 * M]
        torch.add(st.xyzs[:3 * M], float(model.bound), out=x01)
        x01.div_(2.0 * float(model.bound))
        need_tv = L.lib().n2m_grid_binned_workspace_bytes(M, 3, 1, eng.Lv, ho, L.F32, 1)
        ws_tv = L.workspace(dev, need_tv, 1)
        L.call("n2m_grad_total_variation_binned", _p(x01), _p(e1.embeddings), _p(eng.g1), ho, *st.tv, _p(st.seed), M, 3, 1, eng.Lv, eng.S,
               eng.H0, *st.geo[:2], _p(ws_tv), ws_tv.numel(), s)
