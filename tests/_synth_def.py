"""The definition the synthetic-degradation kernels (csrc/synth_degrade.hip) are held to: numpy float64 scalars and Python integers, every
operation and its order written out.  The parameter table is matched bit for bit, the bytes everywhere.

Random words: sample ``i`` at epoch ``e`` reads ``w_k = philox4x32_10(seed, i, 2^32 + 8 e + k)``, k < 8 (the generator of csrc/philox.h,
written out again here).  ``u(r) = (r + 0.5) 2^-32`` (exact), a range draw is ``lo + ((hi - lo) * u(r))`` -- three rounded operations --,
a switch is ``r < threshold`` with thresholds of 2^32, a choice among n is ``(r n) >> 32``:

  w0 = selected, medium on, exposure on, noise on          w4 = a_0, a_1, a_2, gain
  w1 = water type, beta, airlight, range (first draw)      w5 = fx_0, fx_1, fx_2 (>> 30), shot
  w2 = veil_r, veil_g, veil_b, range (second draw)         w6 = fy_0, fy_1, fy_2 (>> 30), read
  w3 = m, gx, gy, gamma                                    w7 = phi_0, phi_1, phi_2 (range (0, 2 pi)), unused

A stage that is switched off leaves beta = 0, (gamma, gain) = (1, 1), (shot, read) = (0, 0) in the row.  ``settings`` is a plain dict:
``type_beta`` (a list of three-tuples, empty: draw ``beta``), and the ranges ``beta airlight veil[3] depth field_mean field_grad
field_amp gamma gain shot read``.

Per pixel (``apply``), in this order:
  J = label / 255, u = (x + 0.5) / W, v = (y + 0.5) / H
  acc = m + gx (u - 0.5); acc = acc + gy (v - 0.5); acc = acc + a_k cos(2 pi (fx_k u + fy_k v) + phi_k) for k = 0, 1, 2
  d = d_lo + (d_hi - d_lo) clamp01(acc)
  beta != 0:                T = exp(-(beta d)), I = J T + B (1 - T)
  gamma != 1:               I = I ** gamma;          then I = gain I
  shot != 0 or read != 0:   I = I + sqrt(max(shot I, 0) + read read) z
  byte = floor(255 clamp01(I) + 0.5)
``z`` is an input: element ``(c H + y) W + x`` of the sample's fp32 noise row, widened."""
import numpy as np

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
ONE = 1 << 32
COUNTER_BASE = 1 << 32
Z_OFFSET = 1 << 33
SEED_TAG = 0x73796E74685F7A31
TWO_PI = np.float64(6.283185307179586)
P = 29
SELECTED, TYPE, M, GX, GY, AMP, FX, FY, PHI, D_LO, D_HI, BETA, VEIL, GAMMA, GAIN, SHOT, READ = (0, 1, 2, 3, 4, 5, 8, 11, 14, 17, 18, 19,
                                                                                              22, 25, 26, 27, 28)
f64 = np.float64


def philox(seed: int, ctr_lo: int, ctr_hi: int):
    """Philox4x32-10 under the two halves of ``seed`` on the counter words of ``(ctr_lo, ctr_hi)``: four 32-bit words."""
    c = [ctr_lo & M32, (ctr_lo >> 32) & M32, ctr_hi & M32, (ctr_hi >> 32) & M32]
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k1) & M32, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return tuple(c)


def counters(epoch: int):
    """The eight high counter words sample ``i`` reads at ``epoch`` (the low word is ``i``)."""
    assert 0 <= epoch < 2 ** 31
    return [COUNTER_BASE + 8 * epoch + k for k in range(8)]


def mix(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def noise_seed(seed: int, i: int, epoch: int) -> int:
    return mix(mix(mix(mix(SEED_TAG) ^ (seed & M64)) ^ (i & M64)) ^ (epoch & M64))


def uniform(r: int):
    return (f64(r) + f64(0.5)) * f64(2.0 ** -32)


def in_range(rng, r: int):
    lo, hi = f64(rng[0]), f64(rng[1])
    span = hi - lo
    step = span * uniform(r)
    return lo + step


def clamp01(v):
    return f64(0.0) if v < 0.0 else (f64(1.0) if v > 1.0 else f64(v))


def param_row(seed: int, epoch: int, i: int, S: dict, th_select: int = ONE, th_medium: int = ONE, th_exposure: int = ONE,
              th_noise: int = ONE) -> np.ndarray:
    """Row of the parameter table for sample ``i`` at ``epoch``: float64 ``[P]``."""
    assert all(0 <= t <= ONE for t in (th_select, th_medium, th_exposure, th_noise))
    w = [philox(seed & M64, i, c) for c in counters(epoch)]
    row = np.zeros(P, dtype=np.float64)
    selected, medium, exposure, noise = w[0][0] < th_select, w[0][1] < th_medium, w[0][2] < th_exposure, w[0][3] < th_noise
    row[SELECTED] = 1.0 if selected else 0.0
    types = S["type_beta"]
    if len(types) > 0:
        t = (w[1][0] * len(types)) >> 32
        beta = [f64(b) for b in types[t]]
    else:
        t = -1
        beta = [in_range(S["beta"], w[1][1])] * 3
    row[TYPE] = float(t)
    airlight = in_range(S["airlight"], w[1][2])
    for c in range(3):
        row[BETA + c] = beta[c] if medium else 0.0
        row[VEIL + c] = clamp01(airlight + in_range(S["veil"][c], w[2][c]))
    d1, d2 = in_range(S["depth"], w[1][3]), in_range(S["depth"], w[2][3])
    row[D_LO], row[D_HI] = (d1, d2) if d1 < d2 else (d2, d1)
    row[M] = in_range(S["field_mean"], w[3][0])
    row[GX] = in_range(S["field_grad"], w[3][1])
    row[GY] = in_range(S["field_grad"], w[3][2])
    for k in range(3):
        row[AMP + k] = in_range(S["field_amp"], w[4][k])
        row[FX + k] = float(w[5][k] >> 30)
        row[FY + k] = float(w[6][k] >> 30)
        row[PHI + k] = in_range((0.0, TWO_PI), w[7][k])
    row[GAMMA] = in_range(S["gamma"], w[3][3]) if exposure else 1.0
    row[GAIN] = in_range(S["gain"], w[4][3]) if exposure else 1.0
    row[SHOT] = in_range(S["shot"], w[5][3]) if noise else 0.0
    row[READ] = in_range(S["read"], w[6][3]) if noise else 0.0
    return row


def param_table(seed: int, epoch: int, idx, S: dict, **th) -> np.ndarray:
    return np.stack([param_row(seed, epoch, int(i), S, **th) for i in idx])


def field(row: np.ndarray, H: int, W: int) -> np.ndarray:
    """The range ``d`` in metres, float64 ``[H, W]``."""
    u = ((np.arange(W, dtype=np.float64) + 0.5) / f64(W))[None, :]
    v = ((np.arange(H, dtype=np.float64) + 0.5) / f64(H))[:, None]
    acc = row[M] + row[GX] * (u - 0.5)
    acc = acc + row[GY] * (v - 0.5)
    for k in range(3):
        turns = row[FX + k] * u + row[FY + k] * v
        acc = acc + row[AMP + k] * np.cos(TWO_PI * turns + row[PHI + k])
    s = np.where(acc < 0.0, 0.0, np.where(acc > 1.0, 1.0, acc))
    return row[D_LO] + (row[D_HI] - row[D_LO]) * s


def apply(label: np.ndarray, row: np.ndarray, z=None):
    """``(bytes, margin)`` for one uint8 ``[3, H, W]`` label under the parameter row: the degraded image, and the smallest distance of
    ``255 I + 0.5`` from an integer over the values that are not clipped (``inf`` if all are).  ``z``: float ``[3, H, W]`` or None."""
    label = np.asarray(label)
    assert label.dtype == np.uint8 and label.ndim == 3 and label.shape[0] == 3
    _, H, W = label.shape
    out = np.empty_like(label)
    margin = np.inf
    beta_on = any(row[BETA + c] != 0.0 for c in range(3))
    d = field(row, H, W) if beta_on else None
    shot, read = row[SHOT], row[READ]
    for c in range(3):
        I = label[c].astype(np.float64) / f64(255.0)
        if row[BETA + c] != 0.0:
            T = np.exp(-(row[BETA + c] * d))
            I = I * T + row[VEIL + c] * (1.0 - T)
        if row[GAMMA] != 1.0:
            I = np.power(I, row[GAMMA])
        I = row[GAIN] * I
        if shot != 0.0 or read != 0.0:
            var = shot * I
            I = I + np.sqrt(np.where(var > 0.0, var, 0.0) + read * read) * np.asarray(z[c], dtype=np.float32).astype(np.float64)
        clipped = (I < 0.0) | (I > 1.0)
        q = f64(255.0) * np.where(I < 0.0, 0.0, np.where(I > 1.0, 1.0, I)) + f64(0.5)
        out[c] = np.floor(q).astype(np.uint8)
        if (~clipped).any():
            free = q[~clipped]
            margin = min(margin, float(np.abs(free - np.rint(free)).min()))
    return out, margin


def degrade(label: np.ndarray, table: np.ndarray, inp: np.ndarray, z=None):
    """``(inp', margin)`` of a batch: the selected samples of ``inp`` replaced, the others kept."""
    out, margin = np.array(inp, copy=True), np.inf
    for j in range(label.shape[0]):
        if table[j, SELECTED] != 0.0:
            out[j], m = apply(label[j], table[j], None if z is None else z[j])
            margin = min(margin, m)
    return out, margin
