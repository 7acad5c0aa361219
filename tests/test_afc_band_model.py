"""The criterion of tests/afc_band.py on the CPU, before any kernel is held to it (tests/test_gpu_afc_demap.py):

  (a) the bound covers the arithmetic: tools/fft_error_bound.py's fp32 model of the kernels' operation order, now with the NCO's rotation in front, stays
      below B = B_fft + B_nco in every bin on the script's adversarial inputs at NCO frequencies up to +-8 kHz; constants() / bin_bound() are what they were;
  (b) the criterion has teeth: that fp32 model, run over the last 20 symbols of one oracle frame of the +3400 Hz capture (and of the 7 dB one) and demapped in fp32 like the kernels
      (hard and soft), passes it -- and the same model with its phase accumulated in fp32 (2 pi f n / fs in float over the frame) fails it, and so does one
      whose symbol stride is off by one sample.  These are models inside this file; the project's code is never altered to try this;
  (c) the caps hold for the reference alone on every capture the GPU tests use (share of decisions inside the hard band <= 1e-3, of values inside the soft
      band <= 1e-2, so a wide band cannot hide a failure), every capture yields >= 12 accepted TFs, the NCO moves on the offset captures, the captures do
      exercise what they are there for (fine time shifts of both signs, a coarse resync after frames were accepted), and the numpy restatement the criterion
      rests on IS the oracle's front end: rotated by the exact frequency it gives or_sdr_demod's bits and or_soft_demap's values.
"""
import numpy as np
import pytest

import afc_band as ab
import oracle_lib as ol
from afc_band import feb

f32 = np.float32


def test_the_bound_covers_the_fp32_model_with_the_nco_in_front():
    c0, c1 = feb.constants(), feb.nco_constants()
    # what test_bench_launch.py holds the guard's constants to has not moved
    assert 6.4e-5 < c0["bin_bound"] < 6.6e-5 and c0["kappa_A"] < c0["kappa_B"] and len(c0) == 11
    # the NCO variant: stage A a general block, the three parts of eps_rot, no B_freq
    assert c1["kappa_A"] == c0["kappa_B"] and c1["B_fft"] > c0["bin_bound"]
    assert c1["B"] == c1["B_fft"] + c1["B_nco"] and c1["B_freq"] == 0.0
    assert abs(c1["eps_rot"] / feb.U - (np.pi + 2 * c1["sincospif_ulp_assumed"] + 1 + np.sqrt(2))) < 1e-4
    assert abs(c1["B_nco"] - np.sqrt(2048.0) * c1["eps_rot"]) < 1e-18
    assert max(feb.nco_bin_bound(k, c1) for k in range(2048)) <= c1["B"] * (1 + 1e-12)
    assert all(feb.nco_bin_bound(k, c1) > feb.bin_bound(k, c0) + c1["B_nco"] * 0.999 for k in range(2048))
    assert max(abs(h) for h in feb.NCO_CHECK_HZ) == 8000 and min(feb.NCO_CHECK_HZ) < 0 < max(feb.NCO_CHECK_HZ)
    r = feb.nco_model_check()
    print("NCO model check: worst bin error %.3e |x|_2 = %.3f of B, %.3f of the bin's own bound, %d cases"
          % (r["worst_bin_error_over_l2"], r["worst_over_bound"], r["worst_over_the_bins_own_bound"], len(r["cases"])))
    assert len(r["cases"]) >= 100 and 0 < r["worst_over_the_bins_own_bound"] <= 1.0 and r["worst_over_bound"] <= 1.0


# ---- (b) the fp32 model of one frame, and two wrong ones ----------------------------------------------------------------------------------------------
SYM_A, SYM_B = 56, 76          # the frame's end: where a phase kept in float has lost the most


_phase = {}


def _fp32_phase(nco_hz):
    """phase[n] = phase[n - 1] + fl(-2 pi f / fs), every addition rounded to float (numpy's cumsum adds in sequence)"""
    if nco_hz not in _phase:
        _phase[nco_hz] = np.concatenate([[f32(0)], np.cumsum(np.full(196607, f32(-2.0 * np.pi * nco_hz / 2048000.0), dtype=f32), dtype=f32)])
    return _phase[nco_hz]


def _rotate(x, nco_hz, l, variant):
    first = ab.FIRST + 2552 * l
    if variant == "kernel":
        return feb.derotate_model(x, feb.nco_inc(nco_hz), first)
    if variant == "stride off by one":                       # the window of symbol l taken to start one sample per symbol later than it does
        return feb.derotate_model(x, feb.nco_inc(nco_hz), ab.FIRST + 2553 * l)
    assert variant == "phase in fp32"                        # 2 pi f n / fs accumulated in float over the frame instead of the 32-bit turn
    a = _fp32_phase(nco_hz)[first:first + 2048]
    cs, sn = np.cos(a.astype(np.float64)).astype(f32), np.sin(a.astype(np.float64)).astype(f32)
    vx, vy = x.real.astype(f32), x.imag.astype(f32)
    return (vx * cs - vy * sn).astype(np.float64) + 1j * (vx * sn + vy * cs).astype(np.float64)


def _model_decisions(samples, nco_hz, variant):
    """-> (bits, soft) [SYM_B - SYM_A - 1][2][1536] in the carrier walk's order, every operation in float32 where the kernels' is"""
    raw = ab.tables()["raw"]
    X, dn = [], []
    for l in range(SYM_A, SYM_B):
        v = _rotate(ab.windows_of(samples, l, l + 1)[0], nco_hz, l, variant)
        vx, vy = v.real.astype(f32), v.imag.astype(f32)
        e = int(np.sum(vx * vx + vy * vy, dtype=f32))                       # the waves' parts are truncated to integers
        dn.append(f32(5.0e-6) * np.sqrt(f32(e)))                           # kSoftNormC * sqrtf(energy)
        X.append(feb.fft2048_model(v)[raw])
    X = np.array(X)
    cx, cy, px, py = (a.astype(f32) for a in (X[1:].real, X[1:].imag, X[:-1].real, X[:-1].imag))
    re = feb.fma32(cx, px, cy * py)                                        # diff_re
    im = -feb.fma32(cx, py, -(cy * px))                                    # -diff_im = Im(cur conj(prev))
    x = np.stack([re, im], axis=1)
    bits = np.stack([~(re > 0), im < 0], axis=1).astype(np.uint8)
    dn = np.array(dn, dtype=f32)
    gain = f32(7.0) / f32(0.94280904)
    scale = (gain * f32(5.0e-6) * f32(5.0e-6)) / (dn[1:] * dn[:-1])        # soft_scale
    soft = np.clip(np.rint((x * scale[:, None, None]).astype(f32)), -7, 7).astype(np.int8)
    return bits, soft


def _outside(got, want, band):
    return int(((got != want) & ~band).sum()), int((got != want).sum())


@pytest.fixture(scope="module", params=["cfo+3400 clean", "cfo+2600 7 dB"])
def frame(request):
    """the last accepted TF of a capture: (name, nco_hz, samples, the reference's decisions and bands of symbols SYM_A + 1 .. SYM_B - 1)"""
    calls, frames = ol.or_frontend_afc_frames(ab.make_capture(ab.CAPTURES[request.param]))
    f = frames[-1]
    assert abs(f.nco_hz - ab.CAPTURES[request.param][2]) < 60  # pulled in: the NCO the frame was de-rotated by is the capture's offset
    x = ab.samples_of(f.buffer)
    return request.param, f.nco_hz, x, ab.Band(ab.windows_of(ab.rotate_quantised(x, f.nco_hz), SYM_A, SYM_B), True)


def test_the_fp32_model_of_the_kernels_passes_the_criterion(frame):
    name, nco_hz, x, band = frame
    bits, soft = _model_decisions(x, nco_hz, "kernel")
    hard_out, hard_diff = _outside(bits, band.bits, band.hard_band)
    soft_out, soft_diff = _outside(soft, band.soft, band.soft_band)
    print("%s, fp32 model at %d Hz: hard (differing %d, in band %d, total %d), soft (differing %d, in band %d, total %d)"
          % (name, nco_hz, hard_diff, band.hard_band.sum(), bits.size, soft_diff, band.soft_band.sum(), soft.size))
    assert hard_out == 0 and soft_out == 0
    assert int(np.abs(soft.astype(int) - band.soft).max()) <= 1
    assert band.soft_band.mean() <= ab.SOFT_CAP and band.hard_band.mean() <= ab.HARD_CAP


@pytest.mark.parametrize("variant", ["phase in fp32", "stride off by one"])
def test_a_subtly_wrong_nco_fails_the_criterion(frame, variant):
    name, nco_hz, x, band = frame
    bits, soft = _model_decisions(x, nco_hz, variant)
    hard_out, hard_diff = _outside(bits, band.bits, band.hard_band)
    soft_out, soft_diff = _outside(soft, band.soft, band.soft_band)
    print("%s, %s at %d Hz: hard differing %d (%d outside the band), soft differing %d (%d outside the band) of %d"
          % (name, variant, nco_hz, hard_diff, hard_out, soft_diff, soft_out, soft.size))
    assert soft_out > 0, "the soft rule lets a wrong NCO through"
    if "clean" in name:      # ... and the decoder would never have noticed: the hard decisions of the clean capture are the oracle's all the same
        assert hard_diff <= 1e-3 * bits.size
    else:                    # at 7 dB decisions lie near zero: the hard rule catches it too
        assert hard_out > 0, "the hard rule lets a wrong NCO through"


# ---- (c) the reference alone on the captures of the GPU tests ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ab.CAPTURES) + ["soft, AFC off, 7 dB"])
def test_caps_hold_for_the_reference_alone(name):
    afc = name in ab.CAPTURES
    iq = ab.make_capture(ab.CAPTURES[name] if afc else ab.SOFT_AFC_OFF_CAPTURE)
    calls, frames = ol.or_frontend_afc_frames(iq, afc=afc, margins=True)
    assert len(frames) >= 12
    ncos = set(c[2] for c in calls)
    if name in ab.OFFSET_CAPTURES:
        assert len(ncos) > 2 and all(f.nco_hz != 0 for f in frames[-8:])
    else:
        assert ncos == {0}
    if "sro" in name:                                           # symbol 75 reaches into the stale tail after a negative fine time shift
        fts = [c[0][3] for c in calls if c[0][0]]
        assert min(fts) < 0 < max(fts)
    if "cut" in name:                                           # a coarse resync after frames were accepted, and frames again behind it, NCO on
        first_ok = next(k for k, c in enumerate(calls) if c[0][0])
        resync = [k for k, c in enumerate(calls) if k > first_ok and c[0][2] != 0]
        assert resync and any(f.call > resync[-1] and f.nco_hz != 0 for f in frames)
    hard = soft = 0
    for t, f in enumerate(frames):
        r = ab.TfReference(f.buffer, f.nco_hz)
        hard += len(r.hard_band)
        soft += len(r.soft_band)
        if t in (0, len(frames) // 2, len(frames) - 1):
            # the restatement is the oracle's front end: rotated by the EXACT frequency, as or_sdr_demod rotates, it gives the oracle's bits, values, margins
            b = ab.Band(ab.windows_of(ab.rotate_exact_hz(ab.samples_of(f.buffer), f.nco_hz)), bool(f.nco_hz))
            assert np.array_equal(b.flat(b.bits), f.bits) and np.array_equal(b.flat(b.soft), f.soft), (name, t)
            m = b.flat(b.x)
            assert np.abs(m - f.margins).max() <= 1e-9 * np.abs(f.margins).max()
            # and the quantised phase moves nothing but decisions inside the band of B_freq's size (the reason the reference rotates by it)
            assert (r.bits != f.bits).mean() <= 1e-3 and np.abs(r.soft.astype(int) - f.soft).max() <= 1
    total = len(frames) * ab.NVALUES
    print("%s: %d TF, NCO values %d, share inside the hard band %.2e, inside the soft band %.2e" % (name, len(frames), len(ncos), hard / total, soft / total))
    assert hard / total <= ab.HARD_CAP and soft / total <= ab.SOFT_CAP
