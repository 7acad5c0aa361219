"""A wideband capture for the tuned mode's tests: the two preset-1 captures of ingest_cases (20 TF) interpolated x2 to 4.096 Msps by exact
band-limited (FFT) interpolation, placed at -856 kHz and +856 kHz -- two neighbouring Band III blocks, 1.712 MHz apart -- and summed.  Test-only
numpy code, nothing of the product.  Computed once per process."""
import functools

import numpy as np

import ingest_cases as cases
import tune_model as tm

RATE = 4096000
OFFSETS = (-856000, 856000)          # channel c carries capture c of ingest_cases
# name -> (format, amplitude of block 0 and of block 1 in rms per rail, in the format's LSB).  Automatic gain in all of them.
VARIANTS = {"cs16_equal": ("cs16", 2000.0, 2000.0), "cs16_plus20": ("cs16", 800.0, 8000.0), "cu8_plus20": ("cu8", 2.5, 25.0)}


@functools.lru_cache(maxsize=None)
def block(i):
    """Capture i at 4.096 Msps, complex, unit rms per rail, moved to OFFSETS[i]."""
    a = cases.direct(i).reshape(-1, 2).astype(np.float64) - 127.0
    x = a[:, 0] + 1j * a[:, 1]
    n = min(cases.direct(k).size // 2 for k in range(len(cases.CAPTURES))) // 2 * 2
    x = x[:n]
    spec = np.fft.fft(x)
    wide = np.zeros(2 * n, np.complex128)
    wide[:n // 2] = spec[:n // 2]
    wide[2 * n - n // 2 + 1:] = spec[n // 2 + 1:]
    wide[n // 2] = wide[2 * n - n // 2] = spec[n // 2] / 2
    y = np.fft.ifft(wide) * 2
    y *= np.exp(2j * np.pi * (OFFSETS[i] / RATE) * np.arange(2 * n))
    return y / np.sqrt(np.mean(np.abs(y) ** 2) / 2)


@functools.lru_cache(maxsize=None)
def raw(variant):
    """The wideband capture in one of VARIANTS: an array of the format's dtype, I and Q interleaved."""
    fmt, a0, a1 = VARIANTS[variant]
    y = a0 * block(0) + a1 * block(1)
    iq = np.stack([y.real, y.imag], axis=1).reshape(-1)
    if fmt == "cs16":
        return np.clip(np.rint(iq), -32768, 32767).astype("<i2")
    return np.clip(np.rint(iq) + 127.0, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def model_output(variant, channel):
    """The model's cu8 at 2.048 Msps of one channel of raw(variant), and the gain it found."""
    m = tm.TuneModel(VARIANTS[variant][0], RATE, OFFSETS[channel], 0)
    return m.push(raw(variant)), m.g
