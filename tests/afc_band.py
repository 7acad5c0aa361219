"""The per-decision criterion that holds the OFDM stage's un-guarded variants -- the software AFC's kernels, hard and soft, and the soft demapper with the
AFC off -- to fp64 (tests/test_afc_band_model.py on the CPU, tests/test_gpu_afc_demap.py on the GPU).  A helper module, no test in it.

A count of differing decisions proves nothing: at 15 dB the Viterbi decoder mends thousands of wrong channel bits per frame.  So the criterion is per decision:
a decision of the kernels may differ from the fp64 reference's ONLY where the reference's own value lies inside the fp32 error band of that very bin.

THE REFERENCE.  The frame buffer the oracle's front end demodulated a TF from (oracle_lib.or_frontend_afc_frames: its 393,216 bytes, stale tail included),
converted like input_sdr.c:60-63, rotated in fp64, the 76 windows at 2656 + 2552 l + 504 transformed by numpy's fp64 FFT, demapped by the rule of
input_sdr.c:132-162 (hard) and oracle/or_soft.c (soft, Q4).  It rotates by the kernels' QUANTISED phase: sample n by exp(-2 pi i (inc n mod 2^32) / 2^32),
inc = llrint(nco_hz 2^32 / 2048000), the integers exact, the angle in fp64 -- NOT by the exact nco_hz as or_sdr_demod does.  So the band needs no B_freq term:
inc is off from nco_hz 2^32 / fs by up to half a unit, which is a frequency offset of up to 2.4e-4 Hz and not an error of the arithmetic; carried through the bound's
own argument (ramp of 1.5e-6 rad inside a window, |x|_1 <= sqrt(2048) |x|_2) it would cost 6.8e-5 |x|_2 per bin, as much as the transform's whole bound.
test_afc_band_model.py ties this numpy restatement to the oracle's C code: rotated by the exact frequency it reproduces or_sdr_demod's bits and or_soft_demap's
values exactly and the oracle's margins to 1e-9.

PER-BIN ERROR.  c, p: the reference's bins of the current and the previous symbol; s_c, s_p: the 2-norms of the two symbols' 2048 (rotated) samples.  The kernels'
bin is off by at most e = B(k) s.  With the NCO off, B(k) = tools/fft_error_bound.py: bin_bound(k), the proven guard's bound (integer samples).  With the NCO on,
B(k) = nco_bin_bound(k) = B_fft(k) + B_nco (the derivation is in that script's docstring, the figures in DESIGN.md section 3):
    B_fft   the transform's bound with stage A taken as a general radix-8 block (its inputs are no longer integers), by the bin's index digits; worst bin 6.7716e-5
    B_nco   sqrt(2048) eps_rot = 2.5776e-5: an error d_n of the rotated samples reaches a bin as at most sum |d_n| <= eps_rot |x|_1 <= eps_rot sqrt(2048) |x|_2;
            eps_rot = (pi + 4 + 1 + sqrt 2) u per sample, u = 2^-24:
              pi u           the turn count: float((int32) t) rounds once, <= u 2^31, times the exact 2^-31: the angle is off by <= pi u rad
              4 u            sincospif, ASSUMED 2 ulp per result (no document under the ROCm installation states it: twice the 1 ulp of the HIP programming
                             guide's table, half of OpenCL's 4 ulp for sinpi / cospi); an ulp is <= 2 u |value|
              (1 + sqrt 2) u the three roundings per component of the product (v.x cs - v.y sn, v.x sn + v.y cs)
    B_freq  none: see THE REFERENCE
    worst bin B = 9.3492e-5.

THE HARD RULE.  T = |c| e_p + |p| e_c + e_c e_p + 2 u (1 + u) (|c| + e_c) (|p| + e_p): the bins' errors carried into cur conj(prev), and the two roundings of
diff_re / diff_im on the computed bins (the script's differential-product part).  A hard decision may differ only where |Re| (first bit) resp. |Im| (second
bit) of the fp64 c conj(p) is <= T.

THE SOFT RULE.  The value is round-half-even(x scale) clamped to +-7, scale = g / (s_c s_p), g = 7 / 0.94280904.  The kernels' scale (device_types.hpp:
soft_scale of dc = C s_c^, dp = C s_p^) has a relative error <= R:
    the energy of a symbol: |v^_n|^2 of the computed rotated samples is within 2 eps_rot (1 + eps_rot) of |x_n|^2; the fp32 sum of the 4096 squares passes every
    term through at most 16 roundings (k_fused.hip: product, 7 fused multiply-adds, x + y, 6 DPP additions = 15; k_fft.hip: product, inner addition, 8
    outer additions, 6 shuffle additions = 16); each of the four waves' parts is truncated to an integer (< 1 each, < 4 in all: 4 / E relative); the sum of
    the four integers is exact, its conversion to float one rounding.  [With the NCO off the samples are integers and all of this is exact.]
    s^ = C sqrtf(E^): half of the above, one ulp (2 u) for the square root, u for the factor:        eps_rot + 8.5 u + 0.5 u + 2 / E + 3 u
    scale^ = K / (dc dp), K = (kSoftGain C) C with kSoftGain = 7.0f / 0.94280904f: 4 roundings in K, one in the product, one ulp (2 u) for the division
    R = (2 eps_rot + 32 u + 2 / E_c + 2 / E_p) (1 + 1e-5)     >= 2 (eps_rot + 12 u) + 2 / E_c + 2 / E_p + 7 u .
The product fl(x^ scale^) adds one rounding.  With y = x scale the reference's scaled value, the kernels' is within
    D = T scale (1 + R) + |y| (R + 2 u)
of it, so a soft value may differ only by 1 and only where y lies within D of a rounding boundary below the clamp (+-0.5, +-1.5, .. +-6.5).

The CAPS (share of reference decisions inside the hard band <= 1e-3 per capture, of values inside the soft band <= 1e-2) keep a wide band from hiding a
failure; test_afc_band_model.py holds them for the reference alone on every capture the GPU tests use."""
import os
import sys

import numpy as np

import oracle_lib as ol

sys.path.insert(0, os.path.join(ol.ROOT, "tools"))
import fft_error_bound as feb  # noqa: E402

U = feb.U
SOFT_GAIN = 7.0 / 0.94280904
HARD_CAP, SOFT_CAP = 1e-3, 1e-2
FIRST = 2656 + 504                    # start of symbol 0's window in the frame buffer; 2552 samples from one window to the next
NSYM = 76
NVALUES = 75 * 3072

_tables = {}


def tables():
    """(shifted bins, raw bins, places) of the carrier walk and the per-bin bounds B(k) of the walk's bins without and with the NCO"""
    if not _tables:
        shifted, raw, rev = ol.carrier_walk()
        c0, c1 = feb.constants(), feb.nco_constants()
        _tables.update(shifted=shifted, raw=raw, rev=rev, eps_rot=c1["eps_rot"],
                       B_off=np.array([feb.bin_bound(int(k), c0) for k in raw]), B_nco=np.array([feb.nco_bin_bound(int(k), c1) for k in raw]))
    return _tables


def samples_of(buffer):
    """input_sdr.c:60-63: (int8)(byte - 127) -> complex128[196608]"""
    b = (np.asarray(buffer, dtype=np.uint8) - np.uint8(127)).view(np.int8).astype(np.float64)
    return b[0::2] + 1j * b[1::2]


def windows_of(x, sym_a=0, sym_b=NSYM):
    """the 2048 samples symbols sym_a .. sym_b - 1 are transformed from: [sym_b - sym_a][2048]"""
    idx = FIRST + 2552 * np.arange(sym_a, sym_b)[:, None] + np.arange(2048)[None, :]
    return x[idx]


def rotate_quantised(x, nco_hz):
    return feb.derotate_exact(x, feb.nco_inc(nco_hz), 0) if nco_hz else x


def rotate_exact_hz(x, nco_hz):
    """what or_sdr_demod does: exp(-2 pi i f n / fs) in fp64 (used only to tie this restatement to the oracle)"""
    n = np.arange(x.size, dtype=np.float64)
    return x * np.exp(-2j * np.pi * float(nco_hz) * n / 2048000.0) if nco_hz else x


class Band:
    """The reference's decisions of symbols sym_a + 1 .. sym_b - 1 of one TF and the band of each: arrays [symbols][2][1536] in the carrier walk's order
    (x: Re / Im of cur conj(prev), positive = bit 0; bits; soft; hard_band, soft_band: True where the kernels may differ)."""

    def __init__(self, windows, nco_on):
        t = tables()
        W = np.asarray(windows, dtype=np.complex128)
        s = np.sqrt(np.sum(W.real ** 2 + W.imag ** 2, axis=1))
        X = np.fft.fft(W, axis=1)[:, t["raw"]]
        c, p = X[1:], X[:-1]
        sc, sp = s[1:, None], s[:-1, None]
        Bk = (t["B_nco"] if nco_on else t["B_off"])[None, :]
        ec, ep = Bk * sc, Bk * sp
        ac, ap = np.abs(c), np.abs(p)
        T = ac * ep + ap * ec + ec * ep + 2 * U * (1 + U) * (ac + ec) * (ap + ep)
        z = c * np.conj(p)
        self.x = np.stack([z.real, z.imag], axis=1)                      # [l][bit][k]
        self.T = T[:, None, :]
        # input_sdr.c:157-158: first bit 0 iff re > 0; second bit 1 iff the stored im = -Im(c conj p) > 0
        self.bits = np.stack([~(z.real > 0), z.imag < 0], axis=1).astype(np.uint8)
        self.hard_band = np.abs(self.x) <= self.T
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = np.where(sc * sp > 0, SOFT_GAIN / (sc * sp), 0.0)
            eps = t["eps_rot"] if nco_on else 0.0
            R = np.where(sc * sp > 0, (2 * eps + 32 * U + 2 / sc ** 2 + 2 / sp ** 2) * (1 + 1e-5), 0.0)
        y = self.x * scale[:, None, :]
        self.y = y
        self.soft = np.clip(np.rint(y), -7, 7).astype(np.int8)          # np.rint: ties to even, like nearbyint and the kernels
        D = self.T * (scale * (1 + R))[:, None, :] + np.abs(y) * (R + 2 * U)[:, None, :]
        m = np.abs(y)
        dist = np.abs(m - (np.clip(np.rint(m - 0.5), 0, 6) + 0.5))     # to the nearest of 0.5 .. 6.5
        self.soft_band = dist <= D
        self.D = D

    def flat(self, a):
        """[75][2][1536] in walk order -> the TF's 230,400 places (FIC then MSC, as the front end stores them)"""
        rev = tables()["rev"]
        out = np.zeros((a.shape[0], 3072), dtype=a.dtype)
        out[:, rev] = a[:, 0]
        out[:, 1536 + rev] = a[:, 1]
        return out.reshape(-1)


class TfReference:
    """What the GPU tests keep per accepted TF: the reference's bits and soft values at the TF's 230,400 places and the places inside either band."""

    def __init__(self, buffer, nco_hz, nco_on=None):
        b = Band(windows_of(rotate_quantised(samples_of(buffer), nco_hz)), bool(nco_hz) if nco_on is None else nco_on)
        self.nco_hz = nco_hz
        self.bits = b.flat(b.bits)
        self.soft = b.flat(b.soft)
        self.hard_band = np.flatnonzero(b.flat(b.hard_band)).astype(np.int32)
        self.soft_band = np.flatnonzero(b.flat(b.soft_band)).astype(np.int32)


class Tally:
    """(differing, in band, total) of a comparison, and the first few decisions that differ OUTSIDE the band"""

    def __init__(self):
        self.differing = self.in_band = self.total = self.outside = self.worst_step = 0
        self.examples = []

    def add(self, got, want, band_idx, where=None):
        got, want = np.asarray(got).astype(np.int32), np.asarray(want).astype(np.int32)
        diff = np.flatnonzero(got != want)
        self.total += got.size
        self.in_band += len(band_idx)
        self.differing += diff.size
        if diff.size:
            self.worst_step = max(self.worst_step, int(np.abs(got[diff] - want[diff]).max()))
            out = np.setdiff1d(diff, band_idx)
            self.outside += out.size
            for i in out[:3]:
                if len(self.examples) < 6:
                    self.examples.append((where, int(i), int(got[i]), int(want[i])))

    def counts(self):
        return (self.differing, self.in_band, self.total)

    def ok(self):
        return self.outside == 0 and self.worst_step <= 1

    def __repr__(self):
        return "(differing %d, in band %d, total %d; outside the band %d, largest step %d%s)" % (
            self.differing, self.in_band, self.total, self.outside, self.worst_step, ", e.g. (TF, place, got, want) %s" % self.examples if self.examples else "")


# ---- the captures both test files use ------------------------------------------------------------------------------------------------------------------
# name: (seed, TFs, cfo_hz, snr_db, skip_samples, sro_ppm, bytes cut out after this many TFs (0: none))
CAPTURES = {
    "cfo+3400 clean": (4601, 24, 3400.0, 1000.0, 0, 0.0, 0),
    "cfo-1700 skip 30000 clean": (4602, 24, -1700.0, 1000.0, 30000, 0.0, 0),
    "cfo-7300 clean": (4603, 28, -7300.0, 1000.0, 0, 0.0, 0),                 # the turn count wraps hundreds of times within a frame
    "cfo+1100 25 dB": (4604, 22, 1100.0, 25.0, 0, 0.0, 0),
    "cfo-260 15 dB": (4605, 20, -260.0, 15.0, 0, 0.0, 0),
    "cfo+2600 7 dB": (4606, 24, 2600.0, 7.0, 0, 0.0, 0),                      # the capture that fills the band
    "cfo 0": (4607, 16, 0.0, 1000.0, 0, 0.0, 0),                              # the NCO stays at 0
    "cfo+900 sro+100ppm": (4608, 24, 900.0, 1000.0, 0, 100.0, 0),             # fine time shifts of both signs: symbol 75 through the view path
    "cfo-900 sro-100ppm": (4609, 24, -900.0, 1000.0, 0, -100.0, 0),
    "cfo+1400, 50,000 bytes cut": (4610, 28, 1400.0, 1000.0, 0, 0.0, 13),     # coarse resync under AFC, stale tail de-rotated by the current frequency
}
OFFSET_CAPTURES = [n for n in CAPTURES if n != "cfo 0"]
SOFT_AFC_OFF_CAPTURE = (4611, 20, 0.0, 7.0, 0, 0.0, 0)                        # the soft demapper with the AFC off, same criterion, the tool's unchanged bound


def make_capture(spec):
    import dabtools_amd as dab
    seed, ntf, cfo, snr, skip, sro, cut = spec
    cfg = dab.synth_preset(1, seed=seed, cif_count0=(37 * seed) % 5000, skip_samples=skip, snr_db=snr, cfo_hz=cfo)
    cfg.channel.sro_ppm = sro
    iq = dab.synth_generate(cfg, ntf)
    if cut:
        iq = np.concatenate([iq[:cut * 393216], iq[cut * 393216 + 50000:]])
    return iq


def reference_of(iq, afc=True):
    """-> (calls, [TfReference per accepted TF]) of the oracle's front end driven call by call"""
    calls, frames = ol.or_frontend_afc_frames(iq, afc=afc)
    return calls, [TfReference(f.buffer, f.nco_hz) for f in frames]
