"""An SDF model of the unbounded recipe (sdf, bound 2 -> contract, two cascades) whose `density` is an analytic signed distance in
CONTRACTED coordinates: a ball of radius 0.4 around the origin (the object, inside the unit box) and, as the background, a closed spherical
shell of thickness 0.2 around contracted radius 1.5 (its two surfaces at 1.4 and 1.6).  Shared by tests/test_sdf_shell_export_gpu.py and
the round trip of tests/test_stage1_contract_gpu.py.

At resolution 48 the outer lattice 2 * linspace(-1, 1, 48)^3 has cells of 4 / 47 = 0.085: the inner surface of the shell (area 4 pi 1.4^2
= 24.6) crosses about 3400 of them, so the exported shell has thousands of faces -- the tests assert at least 300."""
import torch

RESOLUTION = 48
GRID = 32
BALL, SHELL_R, SHELL_HALF = 0.4, 1.5, 0.1
SCALE = 2 - 2 / RESOLUTION


def field(background=True):
    def sdf(p):
        r = p.float().norm(dim=-1)
        d = r - BALL
        if background:
            d = torch.minimum(d, (r - SHELL_R).abs() - SHELL_HALF)
        return {"sigma": d}
    return sdf


def zero_set_distance(p, background=True):
    """Distance of contracted points [N,3] from the zero set of `field` (exact: the field is a distance to spheres)."""
    r = p.double().norm(dim=-1)
    radii = [BALL] + ([SHELL_R - SHELL_HALF, SHELL_R + SHELL_HALF] if background else [])
    return torch.stack([(r - x).abs() for x in radii]).amin(dim=0)


def make_model(background=True, dev="cuda"):
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    torch.manual_seed(0)
    opt = make_options(O=True, sdf=True, bound=2, grid_size=GRID, fused_mlp=True)
    model = NeRFNetwork(opt).to(dev)
    assert opt.contract and model.cascade == 2 and model.bound == 2
    model.density = field(background)
    return model, opt


def export(path, background=True, model=None, **kw):
    """export_stage0(path, resolution=48) on the analytic field -> (model, opt, meshes)."""
    opt = None
    if model is None:
        model, opt = make_model(background)
    return model, opt or model.opt, model.export_stage0(path, resolution=RESOLUTION, **kw)
