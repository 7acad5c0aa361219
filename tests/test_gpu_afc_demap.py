"""The OFDM stage under the software AFC, decision by decision against fp64 (the criterion and its derivation: tests/afc_band.py; the criterion itself is
tested on the CPU by tests/test_afc_band_model.py).

With the AFC on the kernels de-rotate every sample by an NCO (fft_core.hpp: derotate) and the fused kernel gives up its parity guard, so the hard decisions
are plain fp32 comparisons and the soft values fp32 roundings with nothing re-deciding them -- and until this file the suite saw them only through ETI bytes
behind the Viterbi decoder, which mends thousands of wrong channel bits per frame without a trace.  Here, per capture and for each of the four forms of the stage
({hard, soft} x {one kernel, K2 + K2b}):

  * precondition: the per-call integer trace (return value, shifts, FIFO count) and the NCO frequency of every call are the oracle's front end's, driven
    call by call with the tuner rule after every call; the frequency estimate is the oracle's up to whole branch-cut flips of single samples (_assert_trace);
  * every decision of every accepted TF (eng.demapped_tf) against the fp64 reference rotated by the kernels' quantised phase: a hard bit may differ only where
    the reference's |Re| resp. |Im| of cur conj(prev) is inside the bin's error band T, a soft value only by 1 and only where the reference's scaled value is
    within D of a rounding boundary below the clamp;
  * (differing, in band, total) per capture is printed and stands in the assertion message.

The captures (afc_band.CAPTURES): offsets of +3400, -1700 (mid-frame start), -7300 Hz clean (the turn count wraps hundreds of times within a frame), +1100 Hz
at 25 dB, -260 Hz at 15 dB, +2600 Hz at 7 dB (the one that fills the band), no offset (the NCO stays at 0), +-900 Hz with a sampling-rate offset of +-100 ppm
(fine time shifts of both signs: symbol 75 through the view path with the NCO on), and one with 50,000 bytes cut out mid-stream (coarse resync under AFC, the
stale frame-buffer tail de-rotated by the current call's frequency).  Further: the TFs asked for in descending order with the lock-in skip on (deferred frames,
completed on demand, must use their own call's frequency), and the soft demapper with the AFC off at 7 dB under the same per-value criterion with the
transform's unchanged bound (stricter than the count in test_gpu_soft.py)."""
import numpy as np
import pytest

import afc_band as ab
import dabtools_amd as dab

pytestmark = pytest.mark.gpu

FORMS = [("hard", True), ("hard", False), ("soft", True), ("soft", False)]
FORM_IDS = ["hard, one kernel", "hard, K2 + K2b", "soft, one kernel", "soft, K2 + K2b"]

_cache = {}


def _capture(name):
    """(samples, the oracle's calls, a TfReference per accepted TF), computed once for all forms and left unchanged"""
    if name not in _cache:
        afc = name in ab.CAPTURES
        iq = ab.make_capture(ab.CAPTURES[name] if afc else ab.SOFT_AFC_OFF_CAPTURE)
        calls, refs = ab.reference_of(iq, afc=afc)
        assert len(refs) >= 12, (name, len(refs))                         # nothing passes by being empty
        if name in ab.OFFSET_CAPTURES:
            assert len(set(c[2] for c in calls)) > 2, name                # the rule did move the NCO
        _cache[name] = (iq, calls, refs)
    return _cache[name]


@pytest.fixture(scope="module")
def captures():
    return {name: _capture(name) for name in ab.CAPTURES}


def _engine(kind, fused, afc=True):
    eng = dab.Engine(0)
    eng.set_afc(afc)
    eng.set_soft(kind == "soft")
    eng.set_fused(fused)
    return eng


def _assert_trace(eng, b, name, calls):
    ints, ffs = eng.trace(b, len(calls))
    nco = eng.trace_nco(b, len(calls))
    assert len(ints) == len(calls) == len(nco), (name, len(ints), len(calls))
    last_flips = 0
    for k, (want, ffs_want, nco_want) in enumerate(calls):
        assert tuple(int(v) for v in ints[k]) == want, (name, k, list(ints[k]), want)
        assert int(nco[k]) == nco_want, (name, k, int(nco[k]), nco_want)
        # The estimate is the mean of 504 atan2 values (sdr_sync.c's fine_freq_corr).  With the NCO at a multiple of 1 kHz the two samples of a pair, 2048
        # apart, are rotated by the same angle, so a pair of integer samples with Im = 0 and Re < 0 stays ON the branch cut and the last bit of the sine
        # decides between +pi and -pi: the estimate may be off by whole multiples of 1000 / 504 Hz (seen at 7 dB, NCO 2000 Hz), by nothing else.
        # (A call that accepts no frame leaves the previous call's estimate standing.)
        flips = (ffs[k] - ffs_want) * 0.504
        assert abs(flips - round(flips)) < 1e-6 and abs(round(flips)) <= 2, (name, k, ffs[k], ffs_want)
        if want[0]:
            assert (nco_want != 0 and nco_want % 1000 == 0) or round(flips) == 0, (name, k, ffs[k], ffs_want, nco_want)
        else:
            assert round(flips) == last_flips, (name, k, ffs[k], ffs_want)
        last_flips = round(flips)


def _compare(eng, b, kind, refs, order):
    tally = ab.Tally()
    for t in order:
        fic, msc = eng.demapped_tf(b, t)
        got = np.concatenate([fic, msc])
        r = refs[t]
        if kind == "soft":
            tally.add(got, r.soft, r.soft_band, t)
        else:
            assert got.min() >= 0 and got.max() <= 1
            tally.add(got, r.bits, r.hard_band, t)
    return tally


def _report(what, tallies):
    lines = ["%s: (differing, in band, total) per capture" % what] + ["  %-28s %s" % (n, t) for n, t in tallies.items()]
    print("\n".join(lines))
    return "\n".join(lines)


@pytest.mark.parametrize("kind,fused", FORMS, ids=FORM_IDS)
def test_afc_decisions_differ_from_fp64_only_inside_the_error_band(captures, kind, fused):
    names = list(captures)
    eng = _engine(kind, fused)
    eng.set_demod_all(True)                      # every TF through the batch launches (the on-demand path has its own test below)
    eng.decode([captures[n][0] for n in names])
    tallies = {}
    for b, name in enumerate(names):
        iq, calls, refs = captures[name]
        _assert_trace(eng, b, name, calls)
        tallies[name] = _compare(eng, b, kind, refs, range(len(refs)))
        with pytest.raises(dab.DabhipError):
            eng.demapped_tf(b, len(refs))        # and no TF beyond the oracle's
    eng.close()
    msg = _report("AFC on, %s, %s" % (kind, "one kernel" if fused else "K2 + K2b"), tallies)
    assert all(t.ok() for t in tallies.values()), msg
    assert all(t.total == len(captures[n][2]) * ab.NVALUES and t.total >= 12 * ab.NVALUES for n, t in tallies.items()), msg
    if kind == "hard":                           # the NCO at 0 and no decision of this clean capture inside the band: exactly the oracle's bits
        assert tallies["cfo 0"].in_band == 0 and tallies["cfo 0"].differing == 0, msg


@pytest.mark.parametrize("kind,fused", FORMS, ids=FORM_IDS)
def test_deferred_frames_completed_on_demand_use_their_own_calls_frequency(captures, kind, fused):
    """Lock-in skip on (the default): the MSC symbols of the first TFs are not demodulated by the decode; demapped_tf completes them on demand -- asked for in
    descending order, so the early ones come last.  Those are the TFs received while the NCO was still pulling in: each at its own call's frequency."""
    names = ["cfo-7300 clean", "cfo+3400 clean"]
    eng = _engine(kind, fused)
    eng.set_demod_all(False)
    eng.decode([captures[n][0] for n in names])
    deferred = eng.msc_deferred()
    assert deferred >= 9 * len(names)
    tallies = {}
    for b, name in enumerate(names):
        iq, calls, refs = captures[name]
        assert len(set(r.nco_hz for r in refs[:9])) > 2 and refs[0].nco_hz != refs[-1].nco_hz, name      # the deferred TFs have frequencies of their own
        _assert_trace(eng, b, name, calls)
        tallies[name] = _compare(eng, b, kind, refs, reversed(range(len(refs))))
    assert eng.msc_deferred() == deferred
    eng.close()
    msg = _report("AFC on, lock-in skip on, TFs in descending order, %s, %s" % (kind, "one kernel" if fused else "K2 + K2b"), tallies)
    assert all(t.ok() and t.total == len(captures[n][2]) * ab.NVALUES for n, t in tallies.items()), msg


@pytest.mark.parametrize("fused", [True, False], ids=["one kernel", "K2 + K2b"])
def test_soft_demapper_with_the_afc_off_under_the_per_value_criterion(fused):
    name = "soft, AFC off, 7 dB"
    iq, calls, refs = _capture(name)
    assert all(r.nco_hz == 0 for r in refs)
    eng = _engine("soft", fused, afc=False)
    eng.set_demod_all(True)
    eng.decode([iq])
    _assert_trace(eng, 0, name, calls)
    tally = _compare(eng, 0, "soft", refs, range(len(refs)))
    eng.close()
    msg = _report("AFC off, soft, %s" % ("one kernel" if fused else "K2 + K2b"), {name: tally})
    assert tally.ok() and tally.total == len(refs) * ab.NVALUES >= 12 * ab.NVALUES, msg
