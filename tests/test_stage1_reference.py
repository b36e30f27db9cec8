"""Stage-1 caller parity: the reference's UNCHANGED `render_stage1` / `update_triangles_errors` /
`mark_unseen_triangles` (nerf/renderer.py:816-981) and its stage-1 constructor (:123-165) are the oracle.

tests/golden/render_stage1.npz was produced by tests/golden/make_golden_stage1.py = that unchanged Python on the CPU over the scalar C
rasteriser (oracle/nvdiffrast_oracle.py) and the reference's own grid kernels (oracle/_ref).  nvdiffrast is un-vendored: the three raster
operators themselves stay PARITY-UNPINNED (their HIP kernels are checked against the same C functions in tests/test_raster_parity.py);
what is pinned here is the caller around them.

GPU tests:
  * the unchanged reference Python over the HIP facade FILES (backends/nvdiffrast/torch.py, backends/torch_scatter.py,
    backends/_gridencoder.py ...) reproduces the fixture's forward quantities;
  * nerf2mesh_amd's restated renderer (`renderer.render_stage1` ...) reproduces the fixture AND, with gradients, the unchanged reference
    Python on the same device: vertex offsets, colour networks, colour table;
  * the reference's `laplacian_smooth_loss` (nerf/utils.py:176-221) against trainer.UniformLaplacian, value and gradient.
CPU tests: the fixture has content and is what the reference produces today (regenerated live when /root/reference is present).
"""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import render_case as RC   # noqa: E402
import stage1_case as SC   # noqa: E402

GOLD = os.path.join(HERE, "golden")


def fixture():
    return dict(np.load(os.path.join(GOLD, "render_stage1.npz")))


# ------------------------------------------------------------------------------------------------------------------ CPU

def test_stage1_fixture_has_content():
    fx = fixture()
    n = SC.H0 * SC.W0
    assert fx["image"].shape == (n, 3) and fx["trig_id"].shape == (SC.H0, SC.W0)
    cov = (fx["weights_sum"] > 0).mean()
    assert 0.05 < cov < 0.6
    partial = ((fx["weights_sum"] > 1e-3) & (fx["weights_sum"] < 1 - 1e-3)).mean()
    assert partial > 0.01, "no antialiased / supersampled silhouette pixels in the fixture"
    v, f = SC.mesh()
    assert fx["triangles_errors"].shape == (f.shape[0],) and (fx["triangles_errors_cnt"] > 0).sum() > 50
    assert fx["triangles_errors_cnt"].sum() == (fx["trig_id"] >= 0).sum()
    assert 0 < int(fx["unseen_count"]) < f.shape[0]
    # the reference's `mask[trig_id] += 1` quirk (nerf/renderer.py:973): empty pixels carry id -1, which names the LAST face
    assert not np.unpackbits(fx["unseen"])[:f.shape[0]][-1]


def test_stage1_fixture_is_what_the_reference_python_produces_today():
    from oracle import ref_python as RP
    if not RP.available():
        pytest.skip("reference Python not available (neither the checkout nor oracle/_ref/pyref)")
    sys.path.insert(0, GOLD)
    import make_golden_stage1 as MG
    ns = RP.load("ref")
    RP.use_backend("ref")
    with tempfile.TemporaryDirectory() as ws:
        SC.write_workspace(ws)
        model = MG.reference_model(ns, ws)
        live = SC.run_case(model, "cpu", grad=False, ctx=RP.cpu_mode)
    fx = fixture()
    assert set(live) == set(fx)
    for k in fx:
        assert np.array_equal(live[k], fx[k]), k


# ------------------------------------------------------------------------------------------------------------------ GPU

def compare_forward(out, fx, what):
    """Forward quantities against the CPU fixture.  Integer decisions (visible face per pixel, per-face counts, visibility vote) must
    agree except where a pixel centre sits within rounding of an edge: the clip transform is a GEMM (rocBLAS here, MKL there)."""
    rows, bad = [], []

    def check(name, err, limit):
        rows.append(f"  {name:46s} {err:.3g}  (limit {limit:.3g})")
        if not err <= limit:
            bad.append(rows[-1])
    n = SC.H0 * SC.W0
    flips = out["trig_id"] != fx["trig_id"]
    check("trig_id: differing pixels", float(flips.sum()), 4)
    same = ~flips.reshape(-1)
    for key, tol in (("image", 2e-4), ("depth", 2e-4), ("weights_sum", 2e-4)):
        assert out[key].shape == fx[key].shape, f"{key}: shape {out[key].shape}, the reference returns {fx[key].shape}"
        d = np.abs(out[key] - fx[key]).reshape(n, -1).max(-1)
        # a sub-pixel whose edge crossing sits within rounding of the blend decision may take the other branch of antialias: allowed on
        # 3 output pixels at most, and bounded there (measured: 1 pixel at 1.05e-3, everything else <= 2e-5)
        check(f"{key}: output pixels above {tol:g} (agreeing ids)", float((d[same] > tol).sum()), 3)
        check(f"{key}: max abs err on agreeing pixels", float(d[same].max()), 25 * tol)
        check(f"{key}: mean abs err, all pixels", float(d.mean()), 0.1 * tol + 2e-3 * flips.mean())
    check("triangles_errors_cnt: differing faces", float((out["triangles_errors_cnt"] != fx["triangles_errors_cnt"]).sum()), 2 * flips.sum())
    e = np.abs(out["triangles_errors"] - fx["triangles_errors"])
    check("triangles_errors: max abs err on faces with equal counts", float(e[out["triangles_errors_cnt"] == fx["triangles_errors_cnt"]].max()), 1e-3)
    check("loss rel err", abs(float(out["loss"]) - float(fx["loss"])) / float(fx["loss"]), 1e-3)
    check("unseen faces: differing", float((np.unpackbits(out["unseen"]) != np.unpackbits(fx["unseen"])).sum()), 3)
    print(f"\n{what} vs tests/golden/render_stage1.npz:\n" + "\n".join(rows))
    assert not bad, f"{what}:\n" + "\n".join(bad)


def _reference_on_hip(ws, fp16=False):
    from oracle import ref_python as RP
    if not RP.available():
        pytest.skip("reference Python not available (oracle/_ref/pyref not built)")
    sys.path.insert(0, GOLD)
    import make_golden_stage1 as MG
    ns = RP.load("hip")
    RP.use_backend("hip")
    import nerf.renderer as rr
    assert rr.dr.__file__.endswith(os.path.join("backends", "nvdiffrast", "torch.py"))
    model = MG.reference_model(ns, ws, device="cuda", fp16=fp16)
    return ns, model


def _ours(fp16=False, fused=False):
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    opt = make_options(bound=1.0, fp16=fp16, fused_mlp=fused, dt_gamma=0, stage=1)
    model = NeRFNetwork(opt).cuda()
    model.load_state_dict(RC.make_state(False), strict=False)
    v, f = SC.mesh()
    model.init_stage1(torch.from_numpy(v), torch.from_numpy(f))
    return model


@pytest.mark.gpu
def test_unchanged_reference_stage1_over_the_hip_facade():
    with tempfile.TemporaryDirectory() as ws:
        SC.write_workspace(ws)
        ns, model = _reference_on_hip(ws)
        out = SC.run_case(model, "cuda", grad=True, laplacian=ns.utils.laplacian_smooth_loss)
    compare_forward(out, fixture(), "reference-python-on-hip[stage1]")
    assert np.abs(out["grad.vertices_offsets"]).sum() > 0, "no gradient reached the vertex offsets through the HIP antialias"
    assert out["grad_sum.encoder_color.embeddings"] > 0 and np.abs(out["grad.color_net.net.0.weight"]).sum() > 0


@pytest.mark.gpu
def test_restated_stage1_reproduces_the_unchanged_reference():
    from nerf2mesh_amd.trainer import laplacian_smooth_loss
    mine = SC.run_case(_ours(), "cuda", grad=True, laplacian=laplacian_smooth_loss)
    compare_forward(mine, fixture(), "nerf2mesh_amd[stage1]")
    with tempfile.TemporaryDirectory() as ws:
        SC.write_workspace(ws)
        ns, model = _reference_on_hip(ws)
        ref = SC.run_case(model, "cuda", grad=True, laplacian=ns.utils.laplacian_smooth_loss)
    # same device, same kernels underneath: the two callers must agree far below the CPU-vs-GPU tolerances
    assert np.array_equal(mine["trig_id"], ref["trig_id"])
    assert np.array_equal(mine["unseen"], ref["unseen"])
    assert np.array_equal(mine["triangles_errors_cnt"], ref["triangles_errors_cnt"])
    rows = []
    for key in ("image", "depth", "weights_sum", "triangles_errors"):
        d = float(np.abs(mine[key] - ref[key]).max())
        rows.append(f"  {key}: max abs diff {d:.3g}")
        # (the two callers spell the clip transform and the masked write differently -- a GEMM there, broadcast FMAs / index_copy here:
        # fp32 re-association of a handful of terms; measured 7.9e-6 on the image)
        assert d <= 3e-5, rows[-1]
    assert abs(float(mine["laplacian"]) - float(ref["laplacian"])) <= 1e-5 * abs(float(ref["laplacian"]))
    for key in sorted(ref):
        if key.startswith("grad.") or key.startswith("grad_head."):
            assert key in mine, f"no gradient for {key}"
            scale = max(float(np.abs(ref[key]).max()), 1e-30)
            d = float(np.abs(mine[key] - ref[key]).max()) / scale
            rows.append(f"  {key}: rel-to-max diff {d:.3g}")
            # float atomics (interpolate / antialias / table scatter) sum in arrival order, and the weight-gradient GEMMs (contraction over
            # the ~2 400 covered pixels) are BLAS calls whose split-K order is not fixed: measured up to 1.5e-3 on color_net.net.0.weight
            assert d <= 5e-3, rows[-1]
        elif key.startswith("grad_sum."):
            assert abs(mine[key] - ref[key]) <= 1e-4 * ref[key]
    print("\nrestated vs unchanged reference (both on the HIP kernels):\n" + "\n".join(rows))


@pytest.mark.gpu
def test_fp16_stage1_tracks_the_unchanged_reference():
    """`-O` (fp16 autocast shading): restated renderer, unfused and with the fused colour field, against the unchanged reference Python
    on the same device."""
    with tempfile.TemporaryDirectory() as ws:
        SC.write_workspace(ws)
        ns, model = _reference_on_hip(ws, fp16=True)
        ref = SC.run_case(model, "cuda", grad=False)
    for fused in (False, True):
        mine = SC.run_case(_ours(fp16=True, fused=fused), "cuda", grad=False)
        assert np.array_equal(mine["trig_id"], ref["trig_id"])
        d = float(np.abs(mine["image"] - ref["image"]).max())
        print(f"fp16 stage-1 image, fused={fused}: max abs diff to the reference Python {d:.3g}")
        assert d <= (6e-3 if fused else 2e-3)
        # alpha does not pass through the network: only the clip transform's rounding separates the two
        assert float(np.abs(mine["weights_sum"] - ref["weights_sum"]).max()) <= 3e-5
