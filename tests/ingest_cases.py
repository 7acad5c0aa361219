"""Captures for the ingest stage's tests: the two preset-1 captures of smoke() (20 TF) resampled to 2.4 Msps by exact band-limited (FFT)
interpolation -- test-only numpy code, nothing of the product -- and written in the four sample formats.  Computed once per process."""
import functools

import numpy as np

import dabtools_amd as dab
import ingest_model as im
from ingest_model import DTYPES

NTF = 20
RATE = 2400000                      # 196,608 * 75 / 64 = 230,400 samples per TF
CAPTURES = ((11, 0), (12, 50000))   # (seed, skip_samples) as in smoke(); cif_count0 = 100 * seed
# name -> (format, gain at creation)
VARIANTS = {"cs16": ("cs16", 256), "cs16_low_auto": ("cs16", 0), "cf32": ("cf32", 256), "cu8": ("cu8", 256)}


def config(i):
    seed, skip = CAPTURES[i]
    return dab.synth_preset(1, seed=seed, cif_count0=100 * seed, skip_samples=skip)


@functools.lru_cache(maxsize=None)
def direct(i):
    """The capture as the modulator writes it: cu8 at 2.048 Msps."""
    return dab.synth_generate(config(i), NTF)


@functools.lru_cache(maxsize=None)
def resampled(i):
    """The same signal at 2.4 Msps, complex, in cu8 LSB (127 taken off)."""
    a = direct(i).reshape(-1, 2).astype(np.float64) - 127.0
    x = a[:, 0] + 1j * a[:, 1]
    x = x[:x.size // 64 * 64]           # a whole number of 64 -> 75 sample groups
    n = x.size
    n2 = n * 75 // 64
    spec = np.fft.fft(x)
    wide = np.zeros(n2, np.complex128)
    wide[:n // 2] = spec[:n // 2]
    wide[n2 - n // 2 + 1:] = spec[n // 2 + 1:]
    wide[n // 2] = wide[n2 - n // 2] = spec[n // 2] / 2
    return np.fft.ifft(wide) * (n2 / n)


@functools.lru_cache(maxsize=None)
def raw(i, variant):
    """The 2.4 Msps capture in one of VARIANTS: an array of the format's dtype, I and Q interleaved."""
    y = resampled(i)
    iq = np.stack([y.real, y.imag], axis=1).reshape(-1)
    if variant == "cs16":
        return np.clip(np.rint(iq * 256.0), -32768, 32767).astype("<i2")
    if variant == "cs16_low_auto":
        return np.clip(np.rint(iq * 256.0 / 30.0), -32768, 32767).astype("<i2")
    if variant == "cf32":
        return (iq / 128.0).astype("<f4")
    return np.clip(np.rint(iq) + 127.0, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def model_output(i, variant):
    """The model's cu8 at 2.048 Msps of raw(i, variant), and the gain it ran with."""
    fmt, gain = VARIANTS[variant]
    return im.one_shot(fmt, RATE, gain, raw(i, variant))


def random_raw(rng, fmt, n):
    """n samples over the format's whole range with its extremes among them; cf32: beyond full scale, NaN, both infinities and exact .5 ties after
    the scaling by 32768."""
    if fmt == "cf32":
        a = (rng.standard_normal(2 * n) * 0.4).astype("<f4")
        k = max(1, n // 20)
        special = np.array([1.0, -1.0, 0.99999, 3.0, -3.0, np.nan, np.inf, -np.inf, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -1.5 / 32768,
                            32766.5 / 32768, -32767.5 / 32768], "<f4")
        a[rng.integers(0, 2 * n, k)] = rng.choice(special, k)
        return a
    info = np.iinfo(DTYPES[fmt])
    a = rng.integers(info.min, info.max + 1, 2 * n).astype(DTYPES[fmt])
    k = max(1, n // 20)
    a[rng.integers(0, 2 * n, k)] = rng.choice(np.array([info.min, info.max], DTYPES[fmt]), k)
    return a


def samples_for_outputs(L, M, T, k):
    """The fewest input samples of a stream that complete k outputs (k >= 1): output k - 1 needs sample floor((k - 1) M / L) + T/2."""
    return (k - 1) * M // L + T // 2 + 1


def check_stage_ms(handle, entry, want):
    """The contract of dabhip_ingest_stage_ms and dabhip_scan_stage_ms, on the C entry itself: the names in order, min(cap, count) returned and no
    more than that written, null arrays and a null handle refused.  After a push every time is finite and >= 0."""
    import ctypes as C
    fn, n = getattr(dab.lib(), entry), len(want)
    for cap in (0, 1, n - 1, n, n + 3):
        names, ms = (C.c_char_p * (n + 3))(), (C.c_float * (n + 3))(*([-7.0] * (n + 3)))
        got = fn(handle._h, names, ms, cap)
        assert got == min(cap, n), (entry, cap, got)
        assert [names[k].decode() for k in range(got)] == list(want)[:got]
        assert all(np.isfinite(ms[k]) and ms[k] >= 0 for k in range(got)), (entry, list(ms))
        assert all(names[k] is None and ms[k] == -7.0 for k in range(got, n + 3)), (entry, cap)
    names, ms = (C.c_char_p * n)(), (C.c_float * n)()
    for args in ((handle._h, None, ms, n), (handle._h, names, None, n), (None, names, ms, n)):
        assert fn(*args) == -1 and (entry[len("dabhip_"):] + ": null argument") in dab.last_error()
    assert list(handle.stage_ms()) == list(want)
