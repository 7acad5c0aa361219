"""Soft-decision path against its oracle (oracle/or_soft.c) -- VERDICT r3 item 1.

The reference decodes hard decisions only (input_sdr.c:157-158, depuncture.c:36-43), so the soft rule is the product's own
extension; until this round the soft kernels were compared only with each other.  Here:

  * DECODERS, bit-exact: viterbi_fused_kernel<4> (FIC and every MSC code-word shape) fed the very values the oracle decodes,
    through the soft form of the S3 seam (dabhip_dab_set_soft) -- random full-range values, tie-heavy {-1, 0, 1}, all-zero
    (everything punctured / erased: the output is the tie rule's), saturated values with errors; all 64 UEP + 24 EEP shapes.
    Integer arithmetic on both sides: no tolerance.
  * DEMAPPER, stated tolerance: the 4-bit values the OFDM stage (one-kernel and two-kernel) leaves, read back with
    dabhip_engine_demapped_tf, against or_soft_demap's fp64 values on the same captures at 5 and 7 dB:
        no value differs by more than 1, and at most 1e-5 of the values differ at all (measured: 1 .. 4 of 4.1 million per capture)
    (fp32 transform and scale against fp64: a product within ~1e-6 relative of a rounding boundary lands on the other side).
  * END TO END at 5 dB: the oracle's back end fed the GPU's own values reproduces the GPU's ETI bytes exactly (every stage after the
    demapper is integer work), and the oracle's replay on its own values differs only in frames fed by a differing value.
"""
import ctypes as C

import numpy as np
import pytest

import dabtools_amd as dab
import oracle_lib as ol
from test_gpu_parity_r2 import _profile_ensembles

pytestmark = pytest.mark.gpu

VALUE_DIFF_FRACTION = 1e-5         # the stated tolerance of the soft demapper (see the module docstring); measured: 2.4e-7 .. 1.0e-6


def _fic_values(cfg, t, keep, amp=7):
    """Soft FIC of TF t: the four FIC blocks, energy-dispersed, encoded, punctured; +amp for a 0 bit, -amp for a 1 bit."""
    O = ol.oracle()
    out = np.zeros(9216, np.int8)
    for q in range(4):
        f = dab.synth_fibs(cfg, 4 * t + q).copy()
        O.or_descramble(ol._ptr(f), 96)
        bits = ol.or_encode(f)[keep]
        out[2304 * q:2304 * (q + 1)] = np.where(bits == 0, amp, -amp)
    return out


def _keep_mask():
    dep = np.zeros(3096, np.uint8)
    ol.oracle().or_fic_depuncture(ol._ptr(dep), ol._ptr(np.zeros(2304, np.uint8)))
    return dep != 128


def _msc_values(rng, kind):
    if kind == "full":
        return rng.integers(-7, 8, 221184).astype(np.int8)
    if kind == "ties":
        return rng.integers(-1, 2, 221184).astype(np.int8)
    if kind == "zero":
        return np.zeros(221184, np.int8)
    if kind == "saturated":
        v = np.where(rng.integers(0, 2, 221184) == 0, 7, -7).astype(np.int8)
        weak = rng.random(221184) < 0.3
        v[weak] = rng.integers(-2, 3, int(weak.sum())).astype(np.int8)
        return v
    raise ValueError(kind)


@pytest.fixture(params=["wave per code word (k_vitwave.hip)", "lane per code word (viterbi_fused_kernel)"])
def decoder_form(request):
    """Both forms of the decoder, MSC and FIC, pinned through set_decoder_forms (small decodes would run one wave per code word by default)."""
    return "lane" if request.param.startswith("lane") else "wave"


def _assert_forms(obj, form, msc_ran=True):
    assert obj.decoder_forms() == ({form} if msc_ran else set(), {form}), form


def test_soft_decoders_bit_exact_on_identical_values_all_shapes(decoder_form):
    keep = _keep_mask()
    rng = np.random.default_rng(41)
    kinds = ["full", "ties", "zero", "saturated"]
    ensembles = _profile_ensembles()
    covered = set()
    for ei, ens in enumerate(ensembles):
        cfg = dab.synth_preset(1, seed=700 + ei, cif_count0=245 + ei)
        cfg.nsub = len(ens)
        for k, (slform, idx, size, start) in enumerate(ens):
            cfg.sub[k].id = (7 * k + ei) % 64 if len(ens) <= 9 else k * 3
            cfg.sub[k].start_cu = start
            cfg.sub[k].slform = slform
            cfg.sub[k].uep_index = idx if slform == 0 else 0
            cfg.sub[k].eep_protlev = idx if slform == 1 else 0
            cfg.sub[k].size_cu = size
            covered.add((slform, idx, size))
        kind = kinds[ei % len(kinds)]
        od = ol.SoftDab(ol.SOFT_Q4)
        d = dab.Dab(0, soft=True, forms=(decoder_form, decoder_form))
        for t in range(16):
            fic = _fic_values(cfg, t, keep)
            msc = _msc_values(rng, kind)
            od.process(fic, msc)
            d.fic[:] = fic
            d.msc[:] = msc
            _assert_forms(d, decoder_form, d.process_frame() > 0)
        got = np.array(d.frames)
        want = np.array(od.frames)
        assert got.shape == (12, 6144) and want.shape == (12, 6144), (ei, got.shape, want.shape)
        assert np.array_equal(got, want), "ensemble %d (%s values): soft MSC decode differs from the oracle" % (ei, kind)
        od.close()
        d.close()
    assert len(covered) == 64 + 24


def test_soft_fic_decoder_bit_exact_on_arbitrary_values(decoder_form):
    """FIC blocks (768 bits, FIC puncturing) on values that do NOT decode: the FIBs are whatever the tie rule and the metric make of
    them, CRC or not -- the oracle's bytes exactly."""
    O = ol.oracle()
    rng = np.random.default_rng(43)
    d = dab.Dab(0, soft=True, forms=(decoder_form, decoder_form))
    for t, kind in enumerate(["full", "ties", "zero", "saturated", "full", "ties"]):
        fic = _msc_values(rng, kind)[:9216]
        want_fib = np.zeros((12, 32), np.uint8)
        want_ok = np.zeros(12, np.uint8)
        O.or_fic_decode_soft(ol._ptr(fic.astype(np.float32), C.c_float), ol.SOFT_Q4, ol._ptr(want_fib), ol._ptr(want_ok))
        d.fic[:] = fic
        d.msc[:] = 0
        _assert_forms(d, decoder_form, d.process_frame() > 0)
        fibs, ok = d.last_fibs()
        assert np.array_equal(fibs, want_fib), (t, kind)
        assert np.array_equal(ok, want_ok), (t, kind)
    d.close()


def _noisy_streams(snr, ntf=20):
    out = []
    for seed, skip in ((301, 0), (302, 77000)):
        cfg = dab.synth_preset(0, seed=seed, cif_count0=17 * seed, skip_samples=skip, snr_db=snr)
        out.append(dab.synth_generate(cfg, ntf))
    return out


@pytest.mark.parametrize("snr", [5.0, 7.0])
def test_soft_demapper_values_within_the_stated_tolerance_and_eti_given_those_values(snr, decoder_form):
    streams = _noisy_streams(snr)
    eng = dab.Engine(0)
    eng.set_soft(True)
    eng.set_decoder_forms(msc=decoder_form, fic=decoder_form)
    report = {}
    for fused in (True, False):
        eng.set_fused(fused)
        total = eng.decode(streams)
        assert total > 0
        _assert_forms(eng, decoder_form)
        for b, iq in enumerate(streams):
            eti_or, vals, ntf = ol.or_replay_soft(iq, ol.SOFT_Q4, values_tf=64)
            assert ntf == vals.shape[0] and ntf >= 16
            od = ol.SoftDab(ol.SOFT_Q4)
            ndiff = nvals = worst = 0
            for t in range(ntf):
                fic, msc = eng.demapped_tf(b, t)
                g = np.concatenate([fic, msc]).astype(np.int32)
                w = vals[t].astype(np.int32)
                dlt = np.abs(g - w)
                worst = max(worst, int(dlt.max()))
                ndiff += int((dlt != 0).sum())
                nvals += g.size
                od.process(fic, msc)                     # the oracle's back end on the GPU's own values
            assert worst <= 1, "a soft value differs from the fp64 restatement by more than one step"
            assert ndiff <= VALUE_DIFF_FRACTION * nvals, (ndiff, nvals)
            got = eng.eti(b)
            assert np.array_equal(got, np.array(od.frames).reshape(-1, 6144)), "stream %d: ETI differs from the oracle back end fed the same values" % b
            # the oracle's replay on its OWN values: same frame count; frames may differ only where a value did
            assert got.shape == eti_or.shape
            nframes_diff = int((got != eti_or).any(axis=1).sum())
            assert ndiff > 0 or nframes_diff == 0
            assert nframes_diff <= max(2, got.shape[0] // 4)
            report[(fused, b)] = (ndiff, nvals, nframes_diff, got.shape[0])
            od.close()
    print("soft demapper vs oracle at %.0f dB: {(fused, stream): (values differing, values, ETI frames differing, frames)} = %s" % (snr, report))
    eng.close()


def test_soft_equals_hard_oracle_on_a_clean_capture():
    """Where hard decisions decode without errors the soft path must produce the reference's bytes (or_replay = scalar viterbi.c semantics)."""
    cfg = dab.synth_preset(0, seed=311, cif_count0=4990)
    iq = dab.synth_generate(cfg, 20)
    want, _ = ol.or_replay(iq)
    eng = dab.Engine(0)
    eng.set_soft(True)
    eng.decode([iq])
    assert np.array_equal(eng.eti(0), want)
    eng.close()
