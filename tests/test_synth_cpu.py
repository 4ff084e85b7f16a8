"""Host-side tests of the synthetic degradation (hdiff_amd/synth.py, csrc/synth_degrade.hip; no GPU): the definition's Philox and its
counters, the settings' validation, the library's symbols and what the C entries refuse, the definition's closed forms, the rounding
margin of the fixtures the GPU test compares bytes at, and the procedural scenes."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hdiff_amd  # noqa: E402
from hdiff_amd import _capi  # noqa: E402
from hdiff_amd import device_data as DD  # noqa: E402
from hdiff_amd import synth as SY  # noqa: E402
import _augment_def as AD  # noqa: E402
import _synth_def as SD  # noqa: E402
import _synth_fixtures as FX  # noqa: E402

ONE = 1 << 32
SYMBOLS = ("hdiff_synth_params", "hdiff_synth_apply")


# -- 1. random words ------------------------------------------------------------------------------------------------------------------
def test_philox_is_the_integer_philox_of_the_augmentation():
    rng = np.random.default_rng(0)
    cases = [(0, 0, 0), (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1), (7, 3, SD.COUNTER_BASE), (7, 3, SD.COUNTER_BASE + 8 * (2 ** 31 - 1) + 7)]
    cases += [tuple(int(v) for v in rng.integers(0, 2 ** 63, 3)) for _ in range(50)]
    for seed, lo, hi in cases:
        assert SD.philox(seed, lo, hi) == AD.philox4x32_10(seed, lo, hi)


def test_counters_never_meet_the_augmentation():
    top = 2 ** 31 - 1
    assert 2 * top + 1 < SD.COUNTER_BASE == SY.COUNTER_BASE             # batch_assemble reads 2 e and 2 e + 1, e < 2^31
    for e in (0, 1, 2, 12345, top - 1, top):
        c = SD.counters(e)
        assert len(set(c)) == 8 and min(c) >= SD.COUNTER_BASE and max(c) < 2 ** 64
        assert not set(c) & {2 * f + k for f in (0, 1, e, top) for k in (0, 1)}
    assert max(SD.counters(5)) < min(SD.counters(6))                    # and two epochs never share one: 8 e + k is injective
    with pytest.raises(AssertionError):
        SD.counters(2 ** 31)


def test_noise_seed_is_its_own_splitmix():
    from hdiff_amd import schedules
    assert SD.mix(0) == 0xE220A8397B1DCDAF                              # splitmix64's first output for 0
    seen = set()
    for seed in (0, 1, 2 ** 64 - 1):
        for i in range(64):
            for e in (0, 1, 2 ** 31 - 1):
                s = SY.noise_seed(seed, i, e)
                assert s == SD.noise_seed(seed, i, e) and 0 <= s < 2 ** 64
                assert s != schedules.posterior_seed(seed, i, e)
                seen.add(s)
    assert len(seen) == 3 * 64 * 3
    assert SY.Z_OFFSET == SD.Z_OFFSET
    with pytest.raises(ValueError):
        SY.noise_seed(0.5, 0, 0)


# -- 2. the settings ------------------------------------------------------------------------------------------------------------------
def test_synth_validation():
    nan = float("nan")
    for bad in (dict(beta=(nan, 1.0)), dict(gamma=(1.0, nan)), dict(read=nan), dict(range_m=(1.0, float("inf"))),
                dict(beta=(2.0, 1.0)), dict(range_m=(15.0, 0.5)), dict(veil=((0.0, 1.0), (0.5, 0.2), (0.0, 1.0))),
                dict(gamma=(0.0, 1.0)), dict(gamma=(-1.0, 2.0)), dict(gamma=0), dict(beta=(-0.1, 1.0)), dict(shot=(-1e-3, 0.0)),
                dict(range_m=(-1.0, 1.0)), dict(p_noise=1.5), dict(p_medium=nan), dict(p_exposure=True), dict(beta="1"),
                dict(beta=(1, 2, 3)), dict(water_types=["I", "X"]), dict(water_types=["nine"]), dict(water_types=[]),
                dict(water_types={"mine": (0.5, 0.5)}), dict(water_types={"mine": (0.5, 0.0, 0.5)}),
                dict(water_types={"mine": (0.5, 1.5, 0.5)}), dict(water_types={"mine": (0.5, nan, 0.5)}), dict(water_types="I")):
        with pytest.raises(ValueError):
            SY.Synth(**bad)
    for bad in (dict(gamma=(3.0, 1.5)), dict(gain=(nan, 1.0))):
        with pytest.raises(ValueError):
            SY.Synth.lowlight(**bad)
    with pytest.raises(ValueError):
        SY.Synth.haze(tint=-0.1)
    with pytest.raises(ValueError):
        SY.Synth.underwater(water_types=("I", "4"))
    with pytest.raises(ValueError):
        SY.Synth().thresholds(prob=1.1)


def test_synth_presets_dict_eq_repr():
    u, h, l = SY.Synth.underwater(), SY.Synth.haze(), SY.Synth.lowlight()
    assert list(u.water_types) == list(SY.WATER_TYPES) and len(SY.WATER_TYPES) == 10 and u.range_m == (0.5, 15.0)
    for (name, beta), N in zip(u.type_betas(), SY.WATER_TYPES.values()):
        assert beta == tuple(-math.log(v) for v in N) and all(b >= 0 for b in beta)
    assert h.water_types is None and h.beta == (0.4, 1.6) and h.airlight == (0.7, 1.0) and h.veil == ((-0.05, 0.05),) * 3
    assert l.p_medium == 0.0 and l.gamma == (1.5, 3.0) and l.gain == (0.3, 0.9) and l.shot == (0.0, 0.01) and l.read == (0.0, 0.02)
    for s in (u, h, l, SY.Synth(), SY.Synth.underwater(water_types={"mine": (0.5, 0.6, 0.7)})):
        again = SY.Synth.from_dict(s.as_dict())
        assert again == s and again.as_dict() == s.as_dict() and repr(again) == repr(s) and repr(s).startswith("Synth(water_types=")
        assert SY.Synth.from_dict(s) is s
    assert u != h and u != u.as_dict() and SY.Synth(gamma=2) == SY.Synth(gamma=(2, 2))
    assert SY.Synth().thresholds(0.25) == {"th_select": ONE // 4, "th_medium": ONE, "th_exposure": ONE, "th_noise": ONE}
    assert SY.Synth.lowlight().thresholds()["th_medium"] == 0
    S = SY.Synth.underwater().settings()
    assert S.n_types == 10 and S.type_beta[9][2] == -math.log(0.29) and tuple(S.depth) == (0.5, 15.0) and tuple(S.veil[2]) == (0.3, 0.85)


def test_synthetic_plan_of_the_driver():
    from hdiff_amd.diffusion import Train as TR
    base = dict(output_path="out", device_cache=True)
    assert TR.synthetic_plan(base) is None and TR.synthetic_plan(dict(output_path="out")) is None
    u, l = SY.Synth.underwater(), SY.Synth.lowlight()
    plan = TR.synthetic_plan(dict(base, synthetic=u))
    assert plan == {"synthetic": {"atmospheric": u, "underwater": u}, "synthetic_prob": 1.0, "synthetic_val": False}
    assert TR.synthetic_plan(dict(base, synthetic=u.as_dict()))["synthetic"]["underwater"] == u
    plan = TR.synthetic_plan(dict(base, synthetic={"atmospheric": l.as_dict(), "underwater": u}, synthetic_prob=0.5, synthetic_val=True))
    assert plan == {"synthetic": {"atmospheric": l, "underwater": u}, "synthetic_prob": 0.5, "synthetic_val": True}
    assert TR.synthetic_plan(dict(base, synthetic={"underwater": u}))["synthetic"] == {"atmospheric": None, "underwater": u}
    assert TR._synthetic_record(plan)["synthetic"]["atmospheric"] == l.as_dict() and TR._synthetic_record(None) is None
    with pytest.raises(ValueError, match="device_cache=True"):
        TR.synthetic_plan(dict(output_path="out", synthetic=u))
    with pytest.raises(ValueError, match="device_cache=True"):              # refused before anything touches a device
        TR.train(dict(output_path="out", synthetic=u))
    with pytest.raises(ValueError, match="without synthetic"):
        TR.synthetic_plan(dict(base, synthetic_val=True))
    with pytest.raises(ValueError, match="names no stage"):
        TR.synthetic_plan(dict(base, synthetic={"underwater": None}))
    with pytest.raises(ValueError, match="probability"):
        TR.synthetic_plan(dict(base, synthetic=u, synthetic_prob=-0.5))
    with pytest.raises(ValueError, match="gamma"):
        TR.synthetic_plan(dict(base, synthetic=dict(u.as_dict(), gamma=[0.0, 1.0])))
    with pytest.raises(TypeError):
        TR.synthetic_plan(dict(base, synthetic="underwater"))
    assert TR.data_plan(dict(base, seed=3)) == {"device_cache": True, "cache_dir": os.path.join("out", "cache"), "augment": None,
                                                "shuffle": False, "data_seed": 3}            # the data plan itself is what it was


# -- 3. the library -------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hdiff.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(hdiff_[a-z0-9_]+)\s*\(", text))
    lib = hdiff_amd.lib()
    assert lib.hdiff_abi_version() == 6
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (hdiff_[a-z0-9_]+)", out))
    for name in SYMBOLS:
        assert name in declared and name in _capi.EXPORTED_SYMBOLS and name in exported, name
    assert int(re.search(r"HDIFF_SYNTH_PARAMS = (\d+)", text).group(1)) == SY.N_PARAMS == SD.P
    assert int(re.search(r"#define HDIFF_SYNTH_MAX_TYPES (\d+)", text).group(1)) == SY.MAX_TYPES
    assert C.sizeof(SY._Settings) == 8 + 8 * (3 * SY.MAX_TYPES + 2 * 13)               # the struct of the header, field for field
    for key, col in SY.COLUMNS.items():
        c_name = "HDIFF_SYNTH_" + {"amp": "AMP", "selected": "SELECTED"}.get(key, key.upper())
        assert int(re.search(rf"{c_name} = (\d+)", text).group(1)) == col == getattr(SD, key.upper()), key


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    lib = hdiff_amd.lib()
    p = 8          # any non-null address: validation returns before anything is read or launched
    good = SY.Synth.underwater()

    def refused(rc, word):
        assert rc == -1
        assert word in lib.hdiff_last_error().decode(), lib.hdiff_last_error()

    def params(idx=p, B=2, seed=0, epoch=0, S=None, th=(ONE, ONE, ONE, ONE), table=p, zseeds=p, settings="given"):
        S = good.settings() if S is None else S
        return lib.hdiff_synth_params(idx, B, seed, epoch, None if settings is None else C.addressof(S), *th, table, zseeds, None)

    def changed(**kw):
        S = good.settings()
        for name, v in kw.items():
            if name == "n_types":
                S.n_types = v
            elif name == "type_beta":
                S.type_beta[1][2] = v
            elif name.startswith("veil"):
                S.veil[int(name[4])][0], S.veil[int(name[4])][1] = v
            else:
                getattr(S, name)[0], getattr(S, name)[1] = v
        return S

    for name in ("idx", "table", "zseeds", "settings"):
        refused(params(**{name: None}), "null pointer")
    refused(params(B=0), "B = 0")
    refused(params(B=-3), "B = -3")
    for k in range(4):
        th = [ONE] * 4
        th[k] = ONE + 1
        refused(params(th=th), "at most 2^32")
    refused(params(epoch=2 ** 31), "below 2^31")
    refused(params(epoch=2 ** 32 - 1), "below 2^31")
    refused(params(S=changed(n_types=-1)), "n_types = -1")
    refused(params(S=changed(n_types=17)), "n_types = 17")
    refused(params(S=changed(type_beta=-0.5)), "water type 1, channel 2")
    refused(params(S=changed(type_beta=float("nan"))), "water type 1, channel 2")
    for name in ("beta", "airlight", "veil0", "veil1", "veil2", "depth", "field_mean", "field_grad", "field_amp", "gamma", "gain", "shot",
                 "read"):
        refused(params(S=changed(**{name: (2.0, 1.0)})), "lo <= hi")
        refused(params(S=changed(**{name: (1.0, float("nan"))})), "lo <= hi")
        refused(params(S=changed(**{name: (1.0, float("inf"))})), "lo <= hi")
    refused(params(S=changed(beta=(-0.25, 1.0))), "beta from -0.25")
    refused(params(S=changed(depth=(-1.0, 1.0))), "range from -1")
    refused(params(S=changed(gamma=(0.0, 1.0))), "gamma from 0")
    refused(params(S=changed(gamma=(-2.0, 1.0))), "gamma from -2")
    refused(params(S=changed(shot=(-1.0, 1.0))), "at least 0")

    def apply(label=p, table=p, zseeds=p, B=2, H=16, W=16, inp=p):
        return lib.hdiff_synth_apply(label, table, zseeds, B, H, W, inp, None)

    for name in ("label", "table", "zseeds", "inp"):
        refused(apply(**{name: None}), "null pointer")
    refused(apply(B=0), "B = 0")
    for bad in (dict(H=0), dict(H=4097), dict(W=0), dict(W=4097), dict(W=-1)):
        refused(apply(**bad), "between 1 and 4096")


def test_module_refuses_cpu_tensors_and_other_types():
    label = torch.zeros(2, 3, 4, 4, dtype=torch.uint8)
    idx = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="MI355X"):
        SY.degrade(label, idx, synth=SY.Synth.haze(), seed=0, epoch=0)
    with pytest.raises(RuntimeError, match="MI355X"):
        SY.params(idx, synth=SY.Synth.haze(), seed=0, epoch=0)
    with pytest.raises(TypeError):
        SY.params(idx, synth=SY.Synth.haze().as_dict(), seed=0, epoch=0)
    with pytest.raises(RuntimeError, match="MI355X"):
        SY.apply(label, torch.zeros(2, SY.N_PARAMS, dtype=torch.float64), idx, label.clone())


# -- 4. the definition ----------------------------------------------------------------------------------------------------------------
def test_uniform_and_range_draws():
    assert SD.uniform(0) == 2.0 ** -33 and SD.uniform(2 ** 32 - 1) == 1.0 - 2.0 ** -33
    for r in (0, 1, 12345, 2 ** 31, 2 ** 32 - 1):
        assert SD.in_range((0.5, 0.5), r) == 0.5
        assert 0.5 <= SD.in_range((0.5, 15.0), r) <= 15.0
        assert SD.in_range((0.0, 1.0), r) == SD.uniform(r)


def test_parameter_rows_follow_the_settings():
    S = FX.settings_of(FX.VARIANTS["mixed"])
    th = FX.VARIANTS["mixed"].thresholds(0.5)
    rows = SD.param_table(FX.SEED, 3, range(400), S, **th)
    assert rows.shape == (400, SD.P) and rows.dtype == np.float64 and np.isfinite(rows).all()
    for col, p in ((SD.SELECTED, 0.5), (SD.BETA, 0.6)):
        assert abs((rows[:, col] != 0).mean() - p) < 0.1
    assert abs((rows[:, SD.GAMMA] != 1).mean() - 0.5) < 0.1 and abs((rows[:, SD.READ] != 0).mean() - 0.5) < 0.1
    assert set(rows[:, SD.TYPE]) == set(float(t) for t in range(10))
    betas = np.array(S["type_beta"])
    on = rows[:, SD.BETA] != 0
    assert np.array_equal(rows[on, SD.BETA:SD.BETA + 3], betas[rows[on, SD.TYPE].astype(int)])
    assert (rows[:, SD.D_LO] <= rows[:, SD.D_HI]).all() and rows[:, SD.D_LO].min() >= 0.5 and rows[:, SD.D_HI].max() <= 15.0
    for col in (SD.FX, SD.FY):
        assert set(rows[:, col:col + 3].ravel()) == {0.0, 1.0, 2.0, 3.0}
    assert 0 <= rows[:, SD.PHI:SD.PHI + 3].min() and rows[:, SD.PHI:SD.PHI + 3].max() <= 2 * math.pi
    assert (rows[:, SD.VEIL:SD.VEIL + 3] >= 0).all() and (rows[:, SD.VEIL:SD.VEIL + 3] <= 1).all()
    # a sample's row belongs to (seed, epoch, index): not to the batch, and it moves with each of the three
    assert np.array_equal(SD.param_table(FX.SEED, 3, [7, 399, 7], S, **th), rows[[7, 399, 7]])
    assert not np.array_equal(SD.param_row(FX.SEED, 4, 7, S, **th), rows[7])
    assert not np.array_equal(SD.param_row(FX.SEED + 1, 3, 7, S, **th), rows[7])
    haze = SD.param_table(1, 0, range(50), FX.settings_of(FX.VARIANTS["haze"]))
    assert (haze[:, SD.TYPE] == -1).all() and (haze[:, SD.BETA] == haze[:, SD.BETA + 2]).all() and haze[:, SD.BETA].min() >= 0.4
    assert np.ptp(haze[:, SD.VEIL:SD.VEIL + 3], axis=1).max() <= 0.1 and haze[:, SD.VEIL].min() >= 0.65
    low = SD.param_table(1, 0, range(50), FX.settings_of(SY.Synth.lowlight()), **SY.Synth.lowlight().thresholds())
    assert (low[:, SD.BETA:SD.BETA + 3] == 0).all() and low[:, SD.GAMMA].min() >= 1.5


def _row(**kw):
    row = np.zeros(SD.P)
    row[SD.SELECTED], row[SD.GAMMA], row[SD.GAIN], row[SD.M] = 1.0, 1.0, 1.0, 0.5
    for k, v in kw.items():
        col = getattr(SD, k.upper())
        row[col:col + np.size(v)] = v
    return row


def test_closed_forms():
    for H, W in FX.SHAPES:
        label = FX.cache_images(H, W)[0]
        ident, margin = SD.apply(label, _row())                          # gamma = 1, gain = 1, no medium, no noise: the identity
        assert np.array_equal(ident, label) and margin > 0.49
        zero_d, _ = SD.apply(label, _row(beta=(0.3, 1.0, 2.0), veil=(0.1, 0.5, 0.9), d_lo=0.0, d_hi=0.0, amp=(0.1, 0.1, 0.1)))
        assert np.array_equal(zero_d, label)                             # d = 0: T = 1 exactly
        veil = (0.1, 0.5, 0.9)
        far, _ = SD.apply(label, _row(beta=(800.0, 900.0, 1000.0), veil=veil, d_lo=1.0, d_hi=2.0))
        want = np.floor(255.0 * np.array(veil) + 0.5).astype(np.uint8)
        assert np.array_equal(far, np.broadcast_to(want[:, None, None], far.shape))      # beta -> large: the veiling light
        z = np.zeros((3, H, W), dtype=np.float32)
        quiet, _ = SD.apply(label, _row(shot=0.01, read=0.02), z)        # z = 0: noise adds nothing
        assert np.array_equal(quiet, label)
        dark, _ = SD.apply(label, _row(gamma=2.0, gain=0.5))
        assert np.array_equal(dark, np.floor(255.0 * (0.5 * (label / 255.0) ** 2.0) + 0.5).astype(np.uint8))
        batch, _ = SD.degrade(label[None].repeat(2, 0), np.stack([_row(selected=0.0, gamma=2.0), _row(gamma=2.0)]),
                              np.full((2, 3, H, W), 7, dtype=np.uint8))
        assert (batch[0] == 7).all() and np.array_equal(batch[1], SD.apply(label, _row(gamma=2.0))[0])
    # the field: a pure ramp is the ramp, and the range stays inside [d_lo, d_hi]
    d = SD.field(_row(m=0.5, gx=1.0, d_lo=2.0, d_hi=4.0), 2, 4)
    assert np.allclose(d, 2.0 + 2.0 * ((np.arange(4) + 0.5) / 4)[None, :].repeat(2, 0), rtol=0, atol=1e-15)
    d = SD.field(_row(m=0.5, gx=3.0, gy=-3.0, amp=(0.5, 0.5, 0.5), fx=(1, 2, 3), fy=(3, 0, 1), d_lo=2.0, d_hi=4.0), 16, 16)
    assert d.min() == 2.0 and d.max() == 4.0
    assert SD.apply(np.full((3, 1, 1), 255, np.uint8), _row(gain=3.0))[1] == np.inf       # everything clipped: no margin to speak of


def test_noise_free_fixtures_have_their_rounding_margin():
    """A double exp, pow or cos a few ulp off moves 255 I by about 1e-13; with every unclipped value at least 1e-9 from a rounding
    boundary the device's bytes must equal the definition's everywhere (the noisy fixtures are checked beside the device's noise)."""
    checked = 0
    for name, variant, H, W, idx, epoch in FX.fixtures():
        if variant in FX.NOISY:
            continue
        s = FX.VARIANTS[variant]
        label = FX.cache_images(H, W)[list(idx)]
        table = SD.param_table(FX.SEED, epoch, idx, FX.settings_of(s), **s.thresholds())
        _, margin = SD.degrade(label, table, label)
        assert margin >= FX.MARGIN, (name, margin)
        checked += 1
    assert checked == 3 * len(FX.SHAPES)


# -- 5. clean images without files ----------------------------------------------------------------------------------------------------
def test_procedural_scenes_repeat_and_do_not_depend_on_n():
    a = SY.procedural_scenes(5, 24, 40, seed=3)
    assert a.dtype == np.uint8 and a.shape == (5, 3, 24, 40)
    assert np.array_equal(a, SY.procedural_scenes(5, 24, 40, seed=3))
    assert np.array_equal(a, SY.procedural_scenes(6, 24, 40, seed=3)[:5])
    assert not np.array_equal(a, SY.procedural_scenes(5, 24, 40, seed=4))
    assert len({a[i].tobytes() for i in range(5)}) == 5
    assert all(a[i].std() > 10 and len(np.unique(a[i])) > 32 for i in range(5))           # an image, not a flat field
    assert SY.procedural_scenes(0, 8, 8, seed=0).shape == (0, 3, 8, 8)
    assert SY.procedural_scenes(2, 1, 1, seed=0).shape == (2, 3, 1, 1)
    state = np.random.get_state()[1].copy()
    SY.procedural_scenes(1, 8, 8, seed=0)
    assert np.array_equal(state, np.random.get_state()[1])                               # the global generator does not move
    with pytest.raises(ValueError):
        SY.procedural_scenes(1, 0, 8, seed=0)
