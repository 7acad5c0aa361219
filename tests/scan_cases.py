"""Small wideband captures for the block scan's tests, built from the blocks of tune_cases (two preset-1 ensembles at -856 kHz and +856 kHz in a
4.096 Msps capture, unit rms per rail each) plus seeded white noise: the cases of the table the scan's rule was checked on.  Only the first
64 segments of 4096 samples are built.  Test-only numpy code, nothing of the product.  Computed once per process."""
import functools

import numpy as np

import ingest_cases as cases
import scan_model as sm
import tune_cases as tc

RATE = tc.RATE
N = 64 * sm.S
CENTER = 175784000                                    # 5A at -856 kHz, 5B at +856 kHz
# name -> (format, amplitude of block 0, of block 1, of the noise: rms per rail in the format's LSB; clip), and the offsets that must be found
CASES = {
    "cs16_equal": (("cs16", 2000.0, 2000.0, 0.0), (-856000, 856000)),
    "cs16_plus20": (("cs16", 800.0, 8000.0, 0.0), (-856000, 856000)),
    "cu8_plus20": (("cu8", 2.5, 25.0, 0.0), (-856000, 856000)),
    "cs16_plus26": (("cs16", 400.0, 8000.0, 0.0), (856000,)),
    "cs16_plus30": (("cs16", 250.0, 8000.0, 0.0), (856000,)),
    # a block of 1.536 MHz in a capture of 4.096 MHz: in-band SNR = (a1^2 / an^2) (4.096 / 1.536)
    "cs16_one_snr5": (("cs16", 0.0, 2000.0, 2000.0 * np.sqrt(4.096 / 1.536) * 10 ** (-5 / 20)), (856000,)),
    "cs16_one_snr0": (("cs16", 0.0, 2000.0, 2000.0 * np.sqrt(4.096 / 1.536)), ()),
    "cs16_noise": (("cs16", 0.0, 0.0, 3000.0), ()),
    "cu8_noise": (("cu8", 0.0, 0.0, 20.0), ()),
    "cu8_clipped": (("cu8", 0.0, 90.0, 0.0), (856000,)),
}


@functools.lru_cache(maxsize=None)
def raw(name):
    """The capture's first 64 segments in the case's format, I and Q interleaved."""
    (fmt, a0, a1, an), _ = CASES[name]
    y = np.zeros(N, np.complex128)
    if a0:
        y = y + a0 * tc.block(0)[:N]
    if a1:
        y = y + a1 * tc.block(1)[:N]
    if an:
        rng = np.random.default_rng(sum(name.encode()))
        y = y + an * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    iq = np.stack([y.real, y.imag], axis=1).reshape(-1)
    if fmt == "cs16":
        return np.clip(np.rint(iq), -32768, 32767).astype("<i2")
    return np.clip(np.rint(iq) + 127.0, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def model_spectrum(name, nsegments=64):
    """(P, segments) of raw(name) through the model."""
    P, done = sm.spectrum(CASES[name][0][0], raw(name), nsegments)
    P.setflags(write=False)
    return P, done


@functools.lru_cache(maxsize=None)
def direct_spectrum(i, nsegments):
    """ingest_cases.direct(i): one block at the centre of a 2.048 Msps cu8 capture."""
    P, done = sm.spectrum("cu8", cases.direct(i)[:2 * nsegments * sm.S], nsegments)
    P.setflags(write=False)
    return P, done


LONG_NTF = 32                                         # 3 x 2^21 samples per block at 2.048 Msps: sizes the FFT likes


@functools.lru_cache(maxsize=None)
def long_raw():
    """The cs16 capture with the second block 20 dB up once more, 32 TF long (block 1's 50,000 skipped samples are silence at its end): long enough
    for the software AFC to pull a block in (some 7 TF) and for the frames' delay of 15 TF after that."""
    import dabtools_amd as dab
    n = LONG_NTF * 196608
    y = np.zeros(2 * n, np.complex128)
    for i, amp in enumerate((800.0, 8000.0)):
        seed, skip = cases.CAPTURES[i]
        a = dab.synth_generate(dab.synth_preset(1, seed=seed, cif_count0=100 * seed, skip_samples=skip), LONG_NTF).reshape(-1, 2).astype(np.float64) - 127.0
        x = np.zeros(n, np.complex128)
        x[:len(a)] = a[:, 0] + 1j * a[:, 1]
        spec = np.fft.fft(x)
        wide = np.zeros(2 * n, np.complex128)
        wide[:n // 2] = spec[:n // 2]
        wide[2 * n - n // 2 + 1:] = spec[n // 2 + 1:]
        wide[n // 2] = wide[2 * n - n // 2] = spec[n // 2] / 2
        b = np.fft.ifft(wide)
        b *= np.exp(2j * np.pi * (tc.OFFSETS[i] / RATE) * np.arange(2 * n))
        y += (amp / np.sqrt(np.mean(np.abs(b) ** 2) / 2)) * b
    return np.clip(np.rint(np.stack([y.real, y.imag], axis=1).reshape(-1)), -32768, 32767).astype("<i2")
