"""The float64 model of n2m_composite_loss_train (tests/composite_loss_ref.py) against the fp32 chain of the CPU oracle, in all four modes; no
GPU.  This is where the yardstick of tests/test_composite_loss_modes_gpu.py comes from: E_ref(mode), the largest per-ray normalised error of
that serial fp32 chain against the model (printed here; the measured values are in DESIGN 4.24).  Nothing is hard-coded beyond a sanity cap."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import composite_loss_ref as R   # noqa: E402


@pytest.mark.parametrize("mode", R.MODES)
def test_inputs_cover_what_they_claim(mode):
    c = R.edge_case(mode)
    ref, counts = c["ref"], c["rays"][:, 1].tolist()
    assert set(R.EDGE_COUNTS) | {R.LONG} <= set(counts) and counts.count(0) >= 2
    assert sorted((counts[n], idx) for n, idx in c["placed"]) == sorted(R.PLACED)
    assert c["rays"][-1, 0] < c["M"] < c["rays"][-1, 0] + c["rays"][-1, 1]          # the last ray is cut off INSIDE its range
    offs = np.concatenate([[0], np.cumsum(counts)])
    assert np.array_equal(c["rays"][:, 0], offs[:-1])                                  # the ranges tile [0, M + CUT)
    stopped = [n for n in range(c["N"]) if 0 < ref["live"][n] < counts[n]]
    assert len(stopped) > len(R.PLACED)                                                # + stops where the random data puts them
    assert (c["gt"][::3, 3] == 0).all() and (c["gtd"][1::3] == 0).all()
    if mode == "alpha":
        assert c["sig"].max() == np.float32(0.9999)
    R.check_conditions(c, mode, ref)                                                   # (the builder ran it already)


@pytest.mark.parametrize("mode", ["density", "alpha", "depth"])
def test_written_out_backward_is_autograd(mode):
    """The backward the model writes out (the form the entropy mode needs) is float64 autograd where autograd applies."""
    ref = R.edge_case(mode)["ref"]
    assert np.abs(ref["gs_explicit"] - ref["gs"]).max() <= 1e-12 * ref["S"].max()
    assert np.abs(ref["gr_explicit"] - ref["gr"]).max() <= 1e-12 * np.abs(ref["gr"]).max()
    assert np.abs(ref["gs"]).max() > 0 and np.abs(ref["gr"]).max() > 0


def test_entropy_backward_is_the_reference_convention_not_the_derivative():
    """grad_weights[i] multiplies sample i's own suffix term (raymarching.cu:676): the true derivative would weigh each later sample's weight
    with ITS entropy slope.  The two differ visibly on these inputs, so a model that used autograd would be a different function."""
    c = R.edge_case("entropy")
    ref, plain = c["ref"], R.edge_case("density")["ref"]           # same inputs, the loss without the term
    M, g = c["M"], R.SCALE / c["N"]
    ws_term, convention, derivative = np.zeros(M), np.zeros(M), np.zeros(M)
    for n, (a, _) in enumerate(c["rays"].tolist()):
        k = int(ref["live"][n])
        if k:
            w, T, dt = ref["w"][a:a + k], ref["T_after"][n][:k], c["ts"][a:a + k, 1].astype(np.float64)
            gw = R.SCALE * R.LAM_ENT / M * R._entropy_grad(w)
            ws_term[a:a + k] = dt * g * R.LAM_ENT * R._entropy_grad(ref["ws"][n]) * (T - R._suffix(w))      # H(weights_sum): a derivative in both
            convention[a:a + k] = dt * gw * (T - R._suffix(w))
            derivative[a:a + k] = dt * (gw * T - R._suffix(gw * w))
    assert np.abs(plain["gs"] + ws_term + convention - ref["gs"]).max() <= 1e-12 * ref["S"].max()
    assert np.abs(convention - derivative).max() > 1e-2 * np.abs(ref["gs"]).max()


@pytest.mark.parametrize("mode", R.MODES)
def test_model_against_the_fp32_oracle_chain(oracle, mode):
    c = R.edge_case(mode)
    ref, chain = c["ref"], R.oracle_chain(c, mode, oracle)
    assert np.array_equal(chain["live"], ref["live"])                                  # fp32 and float64 stop at the same samples
    for n, (a, cnt) in enumerate(c["rays"].tolist()):
        if cnt == 0 or a + cnt > c["M"]:                                               # empty and cut-off rays: zeros in both
            for r in (ref, chain):
                assert r["live"][n] == 0 and r["ws"][n] == 0 and not r["image"][n].any() and r["depth"][n] == 0
                assert not r["gs"][a:c["M"]][:cnt].any() and not r["gr"][a:c["M"]][:cnt].any()
        else:                                                                          # behind a stop: zeros in both
            for r in (ref, chain):
                assert not r["gs"][a + ref["live"][n]:a + cnt].any() and not r["gr"][a + ref["live"][n]:a + cnt].any()
    assert R.loss_error(chain["loss"], ref) <= 1e-5
    tol = dict(rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(chain["ws"], ref["ws"], **tol)
    np.testing.assert_allclose(chain["image"], ref["image"], **tol)
    np.testing.assert_allclose(chain["depth"], ref["depth"], **tol)
    e_gs, e_gr = R.ray_errors(c, ref, chain["gs"], chain["gr"])
    print(f"E_ref({mode}): grad_sigmas {e_gs:.3e}, grad_rgbs {e_gr:.3e}, loss {R.loss_error(chain['loss'], ref):.3e}")
    for e in (e_gs, e_gr):
        assert np.isfinite(e) and 0 < e < 1e-3, (e_gs, e_gr)                           # a sanity cap: serial fp32 meets it by orders of magnitude


@pytest.mark.parametrize("lams", [(0.0, R.LAM_MASK), (R.LAM_RGB, 0.0)])
def test_one_term_alone(oracle, lams):
    """Each of the rgb and mask terms alone: the model and the chain still agree (the GPU test uses these settings too)."""
    for mode in ("density", "alpha"):
        c = R.edge_case(mode)
        ref = R.model(c, mode, *lams)
        e_gs, e_gr = R.ray_errors(c, ref, *(R.oracle_chain(c, mode, oracle, *lams)[k] for k in ("gs", "gr")))
        assert 0 < e_gs < 1e-3 and e_gr < 1e-3 and (e_gr > 0) == (lams[0] > 0), (mode, e_gs, e_gr)


def test_uniform_background(oracle):
    c = R.edge_case("alpha")
    for bg in (1.0, 0.5):
        ref, chain = R.model(c, "alpha", bg=bg), R.oracle_chain(c, "alpha", oracle, bg=bg)
        assert R.loss_error(chain["loss"], ref) <= 1e-5 and max(R.ray_errors(c, ref, chain["gs"], chain["gr"])) < 1e-3
        assert abs(ref["loss"] - c["ref"]["loss"]) > 1e-3                               # another loss than with the per-ray background


def test_big_case_loss():
    c = R.big_case()
    ref, f32 = R.big_loss(c, torch.float64), R.big_loss(c, torch.float32)
    assert c["N"] == 16 * 1024 + 17 and c["rays"][:, 1].max() == 3 and c["rays"][:, 1].min() == 0 and c["rays"][-1].sum() == c["M"]
    assert 0.01 < ref < 1.0 and abs(f32 - ref) <= 1e-5 * ref
