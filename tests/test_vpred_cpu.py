"""CPU-only checks of v-prediction and min-SNR weighting in the image-conditioned tree: the identities of the definition
(tests/_vpred_def.py) in float64 over the whole default schedule, the weights, what the trainer, the sampler and the helpers refuse,
the driver's host logic (file list, ``prediction.json``, the guard of ``Evaluate``), and the agreement of header, library and binding."""
import os
import re
import subprocess

import pytest
import torch

import hdiff_amd
from hdiff_amd import _capi
from hdiff_amd import autograd as AG
from hdiff_amd import schedules
from hdiff_amd.diffusion import Diffusion as DD
from hdiff_amd.diffusion import Evaluate as EV
from hdiff_amd.diffusion import Train as TR

import _vpred_def as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("hdiff_train_b_tail_fwd", "hdiff_train_b_tail_bwd", "hdiff_v_to_eps")
GAMMA = 5.0


# ----------------------------------------------------------------------------------------------------------------------
# header, library, binding
# ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "hdiff.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(hdiff_[a-z0-9_]+)\s*\(", text))
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hdiff_[a-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported and name in _capi.EXPORTED_SYMBOLS, name
    lib = hdiff_amd.lib()
    assert lib.hdiff_abi_version() == 6          # symbols were added, nothing changed
    assert AG.PREDICTION_CODES == {"eps": 0, "v": 1} and re.search(r"HDIFF_PREDICT_EPS = 0, HDIFF_PREDICT_V = 1", text)
    # the host-side argument checks answer without a device
    assert lib.hdiff_v_to_eps(None, None, None, None, None, 1000, 1, 4, None) != 0
    assert b"null pointer" in lib.hdiff_last_error()
    assert lib.hdiff_train_b_tail_fwd(*([None] * 7), 1000, 1, 4, *([None] * 4), 1, None, 255.0, None) != 0
    assert lib.hdiff_train_b_tail_bwd(*([None] * 7), 1000, 1, 4, *([None] * 4), 1, None, 255.0, None) != 0
    assert b"null pointer" in lib.hdiff_last_error()


# ----------------------------------------------------------------------------------------------------------------------
# the definition's identities, float64, all 1000 indices
# ----------------------------------------------------------------------------------------------------------------------
def _consistent():
    """Per index k one sample: gt, noise, y_t = a gt + s noise and the exact v* = a noise - s gt.  The identities are statements about
    the definition, so a and s are the float64 square roots here (a^2 + s^2 = 1 to float64 rounding); with the fp32 casts the
    kernels use, a^2 + s^2 misses 1 by up to 2^-23 and so would the identities."""
    _, ab = V.schedule()
    sa, s1m = torch.sqrt(ab), torch.sqrt(1.0 - ab)
    t = torch.arange(V.T)
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(V.T, 3, 2, 2, generator=g, dtype=torch.float64) * 2 - 1
    noise = torch.randn(V.T, 3, 2, 2, generator=g, dtype=torch.float64)
    a, s = sa.view(-1, 1, 1, 1), s1m.view(-1, 1, 1, 1)
    return dict(sa=sa, s1m=s1m, t=t, gt=gt, noise=noise, a=a, s=s, y_t=a * gt + s * noise, v=a * noise - s * gt)


def test_v_star_gives_back_noise_and_gt():
    c = _consistent()
    d = V.tail("v", c["v"], c["noise"], c["y_t"], c["gt"], c["t"], c["sa"], c["s1m"], None, 1.0)
    assert float((d["eps_hat"] - c["noise"]).abs().max()) <= 1e-12
    assert float((d["y0"] - c["gt"]).abs().max()) <= 1e-12
    assert float(d["mse"].abs().max()) == 0.0        # the target IS v*
    assert float((d["chain"] + c["s"]).abs().max()) == 0.0 and float(d["chain"].abs().max()) <= 1.0
    # the fp32 casts miss a^2 + s^2 = 1 by their own rounding and no more
    sa32, s1m32 = V.tables32(V.schedule()[1])
    assert float((sa32.double() ** 2 + s1m32.double() ** 2 - 1).abs().max()) < 2.0 ** -22


def test_eps_and_v_forms_of_y0_agree_on_consistent_inputs():
    """With out_eps = eps_hat(out_v) the two forms of y0 are the same image: (y_t - s (a v + s y_t)) / a = ((1 - s^2) y_t - s a v) / a
    = a y_t - s v."""
    c = _consistent()
    g = torch.Generator().manual_seed(1)
    out_v = c["v"] + 0.1 * torch.randn(c["v"].shape, generator=g, dtype=torch.float64)        # an imperfect network
    dv = V.tail("v", out_v, c["noise"], c["y_t"], c["gt"], c["t"], c["sa"], c["s1m"], None, 1.0)
    de = V.tail("eps", dv["eps_hat"], c["noise"], c["y_t"], c["gt"], c["t"], c["sa"], c["s1m"], None, 1.0)
    assert float((de["y0"] - dv["y0"]).abs().max()) <= 1e-12
    d255 = V.tail("v", out_v, c["noise"], c["y_t"], c["gt"], c["t"], c["sa"], c["s1m"], None, 255.0)
    assert float((d255["y0"] * 255.0 - dv["y0"]).abs().max()) <= 1e-12
    # and the amplification this is about: the chain of the eps form is s / a, of the v form s
    assert abs(float((c["s"] / c["a"]).max()) - 157.4) < 0.1 and float(c["s"].max()) <= 1.0
    assert float((de["chain"] + c["s"] / c["a"]).abs().max()) <= 1e-12


# ----------------------------------------------------------------------------------------------------------------------
# weights
# ----------------------------------------------------------------------------------------------------------------------
def test_min_snr_weights():
    betas, ab = V.schedule()
    snr = V.snr(ab)
    w_eps = schedules.min_snr_weights(betas, GAMMA, "eps")
    w_v = schedules.min_snr_weights(betas, GAMMA, "v")
    assert w_eps.dtype == w_v.dtype == torch.float64 and tuple(w_eps.shape) == tuple(w_v.shape) == (V.T,)
    capped = torch.clamp(snr, max=GAMMA)
    for got, want in ((w_eps * snr, capped), (w_v * (snr + 1), capped), (w_eps, V.weights(ab, GAMMA, "eps")), (w_v, V.weights(ab, GAMMA, "v"))):
        assert float(((got - want).abs() / want).max()) <= 4 * 2.0 ** -53
    # the eps weight: capped where snr > gamma -- the first 130 indices of this schedule -- and exactly 1 at the other 870
    assert int((w_eps == 1.0).sum()) == 870 and bool((w_eps[:130] < 1.0).all()) and bool((w_eps[130:] == 1.0).all())
    assert float(snr[129]) > GAMMA > float(snr[130])
    assert bool((w_v < 1.0).all()) and bool((w_v > 0).all())
    assert DD.min_snr_weights is schedules.min_snr_weights and "min_snr_weights" in DD.__all__
    # the trainer holds the fp32 cast, once
    tr = DD.GaussianDiffusionTrainer(torch.nn.Identity(), V.B1, V.BT, V.T, prediction="v", loss_weighting="min_snr", snr_gamma=GAMMA)
    assert tr.mse_weights.dtype == torch.float32 and torch.equal(tr.mse_weights, w_v.float())
    assert "mse_weights" not in tr.state_dict()
    assert DD.GaussianDiffusionTrainer(torch.nn.Identity(), V.B1, V.BT, V.T).mse_weights is None


def test_bad_arguments_are_refused():
    betas, _ = V.schedule()
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), "5", None, True):
        with pytest.raises(ValueError, match="snr_gamma"):
            schedules.min_snr_weights(betas, bad, "eps")
        with pytest.raises(ValueError, match="snr_gamma"):
            DD.GaussianDiffusionTrainer(torch.nn.Identity(), V.B1, V.BT, V.T, loss_weighting="min_snr", snr_gamma=bad)
        with pytest.raises(ValueError, match="snr_gamma"):
            TR.prediction_settings({"snr_gamma": bad})
    for bad in ("x0", "V", "", None, 1):
        with pytest.raises(ValueError, match="prediction"):
            schedules.min_snr_weights(betas, GAMMA, bad)
        with pytest.raises(ValueError, match="prediction"):
            DD.GaussianDiffusionTrainer(torch.nn.Identity(), V.B1, V.BT, V.T, prediction=bad)
        with pytest.raises(ValueError, match="prediction"):
            DD.GaussianDiffusionSampler(torch.nn.Identity(), V.B1, V.BT, V.T, prediction=bad)
        with pytest.raises(ValueError, match="prediction"):
            TR.prediction_settings({"prediction": bad})
    for bad in ("snr", "min-snr", "", 5, True):
        with pytest.raises(ValueError, match="loss_weighting"):
            DD.GaussianDiffusionTrainer(torch.nn.Identity(), V.B1, V.BT, V.T, loss_weighting=bad)
        with pytest.raises(ValueError, match="loss_weighting"):
            TR.prediction_settings({"loss_weighting": bad})
    for bad in (0, 0.0, float("nan"), float("inf"), "255", None, True):
        with pytest.raises(ValueError, match="y0_divisor"):
            DD.GaussianDiffusionTrainer(torch.nn.Identity(), V.B1, V.BT, V.T, y0_divisor=bad)
        with pytest.raises(ValueError, match="y0_divisor"):
            TR.prediction_settings({"y0_divisor": bad})
    with pytest.raises(TypeError, match="unexpected keyword"):
        DD.GaussianDiffusionTrainer(torch.nn.Identity(), V.B1, V.BT, V.T, predict="v")
    x = torch.zeros(1, 3, 2, 2)
    tabs = V.tables32(V.schedule()[1])
    with pytest.raises(ValueError, match="prediction"):
        AG.train_b_loss_tail(x, x, x, x, torch.zeros(1, dtype=torch.long), *tabs, prediction="x0")
    with pytest.raises(ValueError, match="y0_div"):
        AG.train_b_loss_tail(x, x, x, x, torch.zeros(1, dtype=torch.long), *tabs, y0_div=0.0)
    with pytest.raises(ValueError, match="weight_tab"):
        AG.train_b_loss_tail(x, x, x, x, torch.zeros(1, dtype=torch.long), *tabs, weight_tab=torch.ones(3))


def test_defaults_and_recorded_attributes():
    tr = DD.GaussianDiffusionTrainer(torch.nn.Identity(), V.B1, V.BT, V.T)
    assert (tr.prediction, tr.loss_weighting, tr.snr_gamma, tr.y0_divisor) == ("eps", None, 5.0, 255.0)
    assert DD.GaussianDiffusionSampler(torch.nn.Identity(), V.B1, V.BT, V.T).prediction == "eps"
    assert DD.GaussianDiffusionSampler(torch.nn.Identity(), V.B1, V.BT, V.T, prediction="v").prediction == "v"
    assert TR.prediction_settings({}) == {"prediction": "eps", "loss_weighting": None, "snr_gamma": 5.0, "y0_divisor": 255.0}
    assert schedules.PREDICTIONS == ("eps", "v") and schedules.LOSS_WEIGHTINGS == (None, "min_snr")


# ----------------------------------------------------------------------------------------------------------------------
# the drivers' host logic
# ----------------------------------------------------------------------------------------------------------------------
def _config(**kw):
    base = dict(underwater_data_name="HICRD", atmospheric_data_name="LoLI", T=1000, channel=32, channel_mult=[1, 2, 2],
                num_res_blocks=1, dropout=0.15, lr=1e-4, multiplier=2.5, beta_1=1e-4, beta_T=0.02, grad_clip=1.0, batch_size=2,
                epochs_stage_1=3, epochs_stage_2=2, save_checkpoint=2, output_path="unused", pretrained_path=None,
                device_list=["cuda:0"])
    base.update(kw)
    return base


def test_expected_files():
    default = sorted(["ckpt_0_Atmosferic_HICRDLoLI.pt", "ckpt_2_Atmosferic_HICRDLoLI.pt", "ckpt_4_Underwater_HICRDLoLI.pt",
                      "ckpt_5_final_HICRDLoLI.pt", "state_last.pt"])
    assert TR.expected_files(_config()) == default
    assert TR.expected_files(_config(prediction="eps", loss_weighting="min_snr", y0_divisor=1.0)) == default
    assert TR.PREDICTION_FILE == EV.PREDICTION_FILE == "prediction.json"
    assert TR.expected_files(_config(prediction="v")) == sorted(default + ["prediction.json"])


def test_prediction_file_round_trip_and_the_guard(tmp_path):
    settings = TR.prediction_settings(_config(prediction="v", loss_weighting="min_snr", snr_gamma=3, y0_divisor=1))
    assert settings == {"prediction": "v", "loss_weighting": "min_snr", "snr_gamma": 3.0, "y0_divisor": 1.0}
    path = TR.write_prediction_file(str(tmp_path), settings)
    assert path == os.path.join(str(tmp_path), "prediction.json") and EV.read_prediction(path) == settings
    ckpt = os.path.join(str(tmp_path), "ckpt_5_final_HICRDLoLI.pt")          # never opened: only its folder matters
    assert EV.resolve_prediction({}, ckpt) == "v"                            # absent key: the file is read
    assert EV.resolve_prediction({"prediction": "v"}, ckpt) == "v"
    with pytest.raises(ValueError, match="prediction"):
        EV.resolve_prediction({"prediction": "eps"}, ckpt)                   # a v checkpoint is not sampled as eps
    elsewhere = os.path.join(str(tmp_path), "other", "ckpt.pt")              # no file beside it
    assert EV.resolve_prediction({}, elsewhere) == "eps" and EV.resolve_prediction({"prediction": "v"}, elsewhere) == "v"
    with pytest.raises(ValueError, match="prediction"):
        EV.resolve_prediction({"prediction": "x0"}, elsewhere)
    with open(os.path.join(str(tmp_path), "prediction.json"), "w") as f:
        f.write("[]")
    with pytest.raises(ValueError, match="prediction"):
        EV.resolve_prediction({}, ckpt)
