"""Drop-in `_backend` modules for an UNCHANGED reference checkout.

The reference's operator wrappers do `import _raymarching_mob as _backend` / `import _gridencoder as _backend`
/ `import _shencoder as _backend` (raymarching/raymarching.py:9-12, gridencoder/grid.py:9-12,
shencoder/sphere_harmonics.py:9-12) and fall back to a JIT CUDA build only when that import fails.
Putting this directory on sys.path (`nerf2mesh_amd.backends.install()`) makes those imports resolve to the
modules here, which expose the same function tables (same names, positional arguments and in-place
semantics as the pybind11 modules of raymarching/src/bindings.cpp:5-20, gridencoder/src/bindings.cpp:5-9,
shencoder/src/bindings.cpp:5-8) on top of libn2m_hip.so.
"""
import os
import sys


def path():
    return os.path.dirname(os.path.abspath(__file__))


def install(fused_mlp=False):
    """Prepend this directory to sys.path so `import _raymarching_mob` etc. find the HIP-backed modules.
    fused_mlp=True (opt-in): as soon as the reference's `nerf.network` is imported, `fuse_field()` below puts the fused MFMA field behind
    its unchanged NeRFNetwork (an import hook; call `fuse_field(nerf.network.NeRFNetwork)` yourself if the module is already loaded)."""
    if fused_mlp:
        _fuse_on_import()
        track_torch_ema()
    p = path()
    if p not in sys.path:
        sys.path.insert(0, p)
    # a test harness may have parked empty stand-ins under these names (oracle/ref_python.py does, to import the reference Python without
    # its third-party packages): they must not shadow the modules of this directory
    for name in ("mcubes", "nvdiffrast.torch", "nvdiffrast", "torch_scatter", "_raymarching_mob", "_gridencoder", "_shencoder", "_freqencoder"):
        m = sys.modules.get(name)
        if m is not None and getattr(m, "__n2m_stub__", False):
            del sys.modules[name]
    return p


# ------------------------------------------------------------------------------------------------ opt-in: the fused field
def fuse_field(cls):
    """OPT-IN.  The function tables above leave the reference's field as it is written: seven `nn.Linear` calls with K <= 64 per evaluation
    (nerf/network.py:46-54 MLP.forward, :81-108 density / forward, :159-189 geo_feat / rgb) -- on MI355X 3.6 ms of hipBLASLt GEMMs per training
    iteration plus a dozen concat / activation launches (profiles/r05_dropin_kernels.txt), i.e. most of the drop-in path's 10.9 ms.  This
    installs nerf2mesh_amd's fused MFMA field (csrc/mlp.hip: both hash-grid lookups + sigma_net / color_net / specular_net, weights in LDS;
    include/n2m_mlp.h) BEHIND the unchanged class: `cls.forward` and `cls.density` are wrapped so that a call the fused kernels cover --
    device tensors, no individual codes (`c is None`), no tcnn, the two standard encoders, bias-free MLPs of the reference's shapes -- runs
    `nerf2mesh_amd.fused.fused_field / fused_density` (an autograd Function: gradients of both tables and the seven weight matrices arrive
    as `.grad` like any other, so torch.optim.Adam / GradScaler / checkpoints work unchanged), and every other call falls through to
    the reference's own method.  Same parameters, same state_dict, same numerics class as the reference's autocast graph (fp16 operands,
    fp32 accumulation: tests/test_mlp_parity.py); nothing of the reference's source is edited.  Returns cls.

    What the fused forward reads is a COPY of the two tables (`packed_tables`, grafted onto cls), rebuilt when a table's version counter
    or address changes.  Tracked: every write through torch that bumps the counter -- an optimizer step, `load_state_dict`, `p.copy_()` /
    any other in-place op on the parameter.  NOT tracked: a write through `param.data` (`param.data.copy_(...)`), which leaves the counter
    alone.  torch_ema's `copy_to` / `restore` write exactly so: `install(fused_mlp=True)` wraps them (`track_derived_copies`), and any
    other such writer has to call `model.invalidate_derived_copies()` (grafted too) itself -- without it the forward goes on reading the
    tables as they were before the write."""
    import torch
    if getattr(cls, "_n2m_fused_field", False):
        return cls
    ref_forward, ref_density = cls.forward, cls.density

    def _prepare(self):
        ok = getattr(self, "_n2m_fuse_ok", None)
        if ok is None:
            try:
                e1, e2 = self.encoder, self.encoder_color
                shapes = [tuple(l.weight.shape) for m in (self.sigma_net, self.color_net, self.specular_net) for l in m.net]
                ok = (not getattr(self.opt, "tcnn", False) and getattr(self, "individual_dim", 0) == 0
                      and all(l.bias is None for m in (self.sigma_net, self.color_net, self.specular_net) for l in m.net)
                      and shapes == [(32, 19), (1, 32), (64, 35), (64, 64), (6, 64), (32, 6), (3, 32)]
                      and e1.embeddings.shape[1] == 1 and e2.embeddings.shape[1] == 2 and e1.num_levels == 16 and e2.num_levels == 16
                      and e1.input_dim == 3 and e2.input_dim == 3)
                if ok:
                    from nerf2mesh_amd.network import NeRFNetwork as _Ours
                    for e in (e1, e2):          # host copy of the level offsets: lets the two tables share one lookup / one backward fill
                        if not hasattr(e, "host_offsets"):
                            e.host_offsets = [int(v) for v in e.offsets.detach().cpu().tolist()]
                    if not hasattr(type(self), "packed_tables"):
                        type(self).packed_tables = _Ours.packed_tables      # the 8-byte-row copy of both tables the fused lookup gathers from
                    if not hasattr(type(self), "invalidate_derived_copies"):
                        type(self).invalidate_derived_copies = _Ours.invalidate_derived_copies      # ... and the way to make it forget them
                    from nerf2mesh_amd.network import derived_copy_holders
                    derived_copy_holders.add(self)
            except Exception:
                ok = False
            self._n2m_fuse_ok = ok
        return ok

    def forward(self, x, d, c=None, shading="full"):
        if c is None and x.is_cuda and shading in ("full", "diffuse", "specular") and _prepare(self):
            from nerf2mesh_amd.fused import fused_field
            lead = x.shape[:-1]
            sigma, color, specular = fused_field(self, x.reshape(-1, 3), d.reshape(-1, 3), shading)
            return sigma.view(lead), color.view(*lead, 3), (None if specular is None else specular.view(*lead, 3))
        return ref_forward(self, x, d, c, shading)

    def density(self, x):
        if x.is_cuda and not x.requires_grad and _prepare(self):
            from nerf2mesh_amd.fused import fused_density
            return {"sigma": fused_density(self, x.reshape(-1, 3)).view(x.shape[:-1])}
        return ref_density(self, x)

    forward.__doc__ = "nerf2mesh_amd.backends.fuse_field: fused MFMA field when covered, else " + (ref_forward.__qualname__)
    cls.forward, cls.density = forward, density
    cls._n2m_fused_field = True
    cls._n2m_reference_forward, cls._n2m_reference_density = ref_forward, ref_density
    return cls


def track_derived_copies(ema_cls):
    """Wrap `ema_cls.copy_to` and `ema_cls.restore` (torch_ema.ExponentialMovingAverage, or a class with its method names) so that every
    live field one of whose hash tables is among the parameters just written forgets its derived copies
    (`invalidate_derived_copies`): both methods write `param.data.copy_(...)`, which no version counter records.  The parameters are
    the `parameters` argument, else what the instance tracks (`_get_parameters`, `_params` or `params`); an instance that shows neither
    invalidates every live field (a spurious rebuild costs one pass over the tables at the next forward).  Returns ema_cls."""
    import functools
    if getattr(ema_cls, "_n2m_tracks_derived_copies", False):
        return ema_cls

    def written(ema, parameters):
        if parameters is not None:
            return parameters
        get = getattr(ema, "_get_parameters", None)
        if get is not None:
            return list(get(None))
        for name in ("_params", "params"):
            if isinstance(getattr(ema, name, None), (list, tuple)):
                return list(getattr(ema, name))
        return None

    def wrap(method):
        @functools.wraps(method)
        def wrapped(self, parameters=None):
            if parameters is not None:
                parameters = list(parameters)          # (a generator: the method and the scan below both walk it)
            out = method(self, parameters)
            from nerf2mesh_amd.network import derived_copy_holders
            ps = written(self, parameters)
            ids = None if ps is None else {id(p) for p in ps}
            for model in list(derived_copy_holders):
                if ids is None or id(model.encoder.embeddings) in ids or id(model.encoder_color.embeddings) in ids:
                    model.invalidate_derived_copies()
            return out
        return wrapped

    ema_cls.copy_to, ema_cls.restore = wrap(ema_cls.copy_to), wrap(ema_cls.restore)
    ema_cls._n2m_tracks_derived_copies = True
    return ema_cls


def track_torch_ema():
    """track_derived_copies on torch_ema.ExponentialMovingAverage -- the class the reference Trainer swaps the averaged weights in and out
    with (nerf/utils.py:1250-1252) -- when that package is installed; False when it is not (nothing to wrap: no hard dependency)."""
    try:
        import torch_ema
    except ImportError:
        return False
    track_derived_copies(torch_ema.ExponentialMovingAverage)
    return True


def unfuse_field(cls):
    """Undo fuse_field (tests: the same class with and without the fused field)."""
    if getattr(cls, "_n2m_fused_field", False):
        cls.forward, cls.density = cls._n2m_reference_forward, cls._n2m_reference_density
        cls._n2m_fused_field = False
    return cls


def _fuse_on_import():
    m = sys.modules.get("nerf.network")
    if m is not None and hasattr(m, "NeRFNetwork"):
        fuse_field(m.NeRFNetwork)
        return
    import importlib.abc
    import importlib.util

    class _Hook(importlib.abc.MetaPathFinder):
        busy = False

        def find_spec(self, name, path_, target=None):
            if name != "nerf.network" or _Hook.busy:
                return None
            _Hook.busy = True
            try:
                spec = importlib.util.find_spec(name)
            finally:
                _Hook.busy = False
            if spec is None or spec.loader is None:
                return None
            loader, exec_module = spec.loader, spec.loader.exec_module

            def patched_exec(module):
                exec_module(module)
                if hasattr(module, "NeRFNetwork"):
                    fuse_field(module.NeRFNetwork)
            try:
                loader.exec_module = patched_exec
            except Exception:
                return None
            return spec

    if not any(type(h).__name__ == "_Hook" for h in sys.meta_path):
        sys.meta_path.insert(0, _Hook())
