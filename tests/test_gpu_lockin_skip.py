"""Lock-in skip: the OFDM stage does not demodulate the MSC symbols of transmission frames that cannot be locked (control_plane.hpp:
lockin_deferred -- the first 9 - okcount TFs of a stream that is not locked when a decode or a session's segment starts).  tests/test_lockin_rule.py
shows on the CPU that the reference's back end never reads them; here the engine: same ETI bytes as the oracle and as itself with the skip switched
off (set_demod_all), the number of deferred TFs the rule gives, demapped_tf completing deferred TFs on demand, sessions whose lock-in straddles
segment boundaries, a lock loss in front of a boundary, and batches of unequal and very short streams."""

import numpy as np
import pytest

import dabtools_amd as dab
import oracle_lib as ol
from oracle_lib import _ptr

pytestmark = pytest.mark.gpu


def _capture(seed, ntf, snr=1000.0, skip=0, preset=1):
    return dab.synth_generate(dab.synth_preset(preset, seed=seed, cif_count0=(53 * seed) % 5000, snr_db=snr, skip_samples=skip), ntf)


def _good_flags(iq):
    """Per 262,144-byte call of the capture: None (no TF demodulated) or whether all 12 FIBs of its TF pass their CRC -- the oracle's front end and FIC decode."""
    O = ol.oracle()
    S = O.or_sdr_new()
    fic, msc = np.zeros(dab.FIC_BITS, np.uint8), np.zeros(dab.MSC_BITS, np.uint8)
    fibs, ok = np.zeros((12, 32), np.uint8), np.zeros(12, np.uint8)
    out = []
    for off in range(0, iq.size - dab.CHUNK_BYTES + 1, dab.CHUNK_BYTES):
        if O.or_sdr_demod(S, _ptr(iq[off:off + dab.CHUNK_BYTES]), dab.CHUNK_BYTES, _ptr(fic), _ptr(msc)):
            O.or_fic_decode(_ptr(fic), _ptr(fibs), _ptr(ok))
            out.append(bool((ok != 0).all()))
        else:
            out.append(None)
    O.or_sdr_free(S)
    return out


def _expected_deferred(flags, boundaries):
    """TFs the rule defers in each segment of a session fed up to boundaries[i] bytes (a one-shot decode: one boundary), the lock rule of dab.c:46-61
    followed by the test itself: ten good TFs in a row lock, a bad one unlocks and clears the count."""
    locked, okcount, call, out = False, 0, 0, []
    for end in boundaries:
        seg = [f for f in flags[call:end // dab.CHUNK_BYTES] if f is not None]
        call = max(call, end // dab.CHUNK_BYTES)
        out.append(dab.host_lockin_deferred(locked, okcount, len(seg)))
        for good in seg:
            okcount = okcount + 1 if good else 0
            locked = good and (locked or okcount >= 10)
    return out


def test_one_shot_equals_oracle_and_demod_all():
    """(a) clean and noisy captures (5 dB: FIBs fail now and then, lock comes late or never; 9 dB: frames with decoding errors in them): ETI == oracle ==
    the engine with the skip off; the clean ones defer nine TFs each, demod-all none."""
    caps = [_capture(2101, 24), _capture(2102, 26, skip=70001), _capture(2103, 24, snr=5.0), _capture(2104, 25, snr=5.0, skip=1234), _capture(2504, 31, snr=5.0),
            _capture(2105, 24, snr=9.0)]
    wants = [ol.or_replay(c)[0] for c in caps]
    assert all(len(w) >= 4 * 8 for w in wants[:2]) and len(wants[4]) > 0 and len(wants[5]) > 0
    expect = [_expected_deferred(_good_flags(c), [c.size])[0] for c in caps]
    assert expect[:2] == [9, 9] and all(e >= 9 for e in expect)
    eng = dab.Engine(0)
    for demod_all in (False, True, False):
        eng.set_demod_all(demod_all)
        assert eng.decode(caps) == sum(len(w) for w in wants)
        assert eng.msc_deferred() == (0 if demod_all else sum(expect)), demod_all
        for b, w in enumerate(wants):
            assert np.array_equal(eng.eti(b), w), (demod_all, b)
    assert eng.decode(caps[:2]) == len(wants[0]) + len(wants[1]) and eng.msc_deferred() == 18
    eng.close()


@pytest.mark.parametrize("mode", ["guard0", "guard1", "guard2", "soft"])
@pytest.mark.parametrize("fused", [True, False])
def test_demapped_tf_completes_deferred_frames_on_demand(mode, fused):
    """(b) demapped_tf of every TF, asked for in descending order (the early, deferred ones last: completion on demand supplies them, not luck), equal
    between the skipping engine and the one that demodulates everything; the deferred count and the decisions' count stay what they were."""
    caps = [_capture(2201, 24), _capture(2202, 24, snr=5.0, skip=50000)]
    ntf = [sum(t.ok for t in ol.or_replay(c)[1]) for c in caps]
    assert min(ntf) >= 20
    eng = dab.Engine(0)
    if mode == "soft":
        eng.set_soft(True)
    else:
        eng.set_parity_guard(int(mode[-1]))
    eng.set_fused(fused)
    got = {}
    for demod_all in (False, True):
        eng.set_demod_all(demod_all)
        total = eng.decode(caps)
        assert total > 0
        deferred, stats = eng.msc_deferred(), eng.guard_stats()
        assert deferred == (0 if demod_all else 18)
        if mode in ("guard1", "guard2"):
            assert stats[1] == sum(ntf) * 230400
        got[demod_all] = {(b, t): eng.demapped_tf(b, t) for b in range(len(caps)) for t in reversed(range(ntf[b]))}
        assert eng.msc_deferred() == deferred and eng.guard_stats()[1] == stats[1]
        with pytest.raises(dab.DabhipError):
            eng.demapped_tf(0, ntf[0])
    for key, (fic, msc) in got[True].items():
        assert np.array_equal(got[False][key][0], fic), ("fic", key)
        assert np.array_equal(got[False][key][1], msc), ("msc", key)
    assert any(msc.any() for (b, t), (fic, msc) in got[False].items() if t < 9)        # the deferred TFs' values are there, not an empty buffer
    eng.close()


def _feed_session(caps, seg_tfs, demod_all=False):
    """-> (frames per stream, deferred TFs per segment, byte boundaries)"""
    st = dab.Stream(len(caps), 0)
    st.set_demod_all(demod_all)
    frames, deferred, bounds = [[] for _ in caps], [], []
    at = 0
    size = max(c.size for c in caps)
    sizes = [k * dab.TF_BYTES for k in seg_tfs]
    while at < size:
        n = sizes[len(bounds)] if len(bounds) < len(sizes) else size - at
        st.feed([c[min(at, c.size):min(at + n, c.size)] for c in caps])
        at += n
        bounds.append(at)
        deferred.append(st.msc_deferred())
        for b in range(len(caps)):
            frames[b].append(st.eti(b))
    st.close()
    return [np.concatenate(f) for f in frames], deferred, bounds


def test_session_with_lock_in_across_segment_boundaries():
    """(c) uneven segments: the nine dead TFs of each stream are spread over several segments, okcount carried from one to the next."""
    caps = [_capture(2301, 30), _capture(2302, 30, skip=90000)]
    wants = [ol.or_replay(c)[0] for c in caps]
    eng = dab.Engine(0)
    assert eng.decode(caps) == sum(len(w) for w in wants)
    one_shot = [eng.eti(b) for b in range(2)]
    eng.close()
    seg_tfs = [3, 1, 7, 2, 1, 1, 4, 2, 5]
    frames, deferred, bounds = _feed_session(caps, seg_tfs)
    for b, w in enumerate(wants):
        assert np.array_equal(frames[b], w) and np.array_equal(one_shot[b], w), b
    flags = [_good_flags(c) for c in caps]
    expect = [sum(x) for x in zip(*[_expected_deferred(f, bounds) for f in flags])]
    assert deferred == expect and sum(deferred) == 18, (deferred, expect)
    assert sum(1 for d in deferred if d) >= 3                       # lock-in did straddle boundaries
    frames_all, deferred_all, _ = _feed_session(caps, seg_tfs, demod_all=True)
    assert sum(deferred_all) == 0 and all(np.array_equal(a, w) for a, w in zip(frames_all, wants))


def test_lock_loss_in_front_of_a_segment_boundary():
    """(d) the FIC symbols of one TF after lock destroyed: the session's segment behind the loss defers 9 - okcount TFs (boundary right behind the
    loss: nine; three calls later: fewer); one-shot, nothing is deferred beyond the first nine.  ETI == the oracle's replay every time."""
    iq = _capture(2401, 40).copy()
    rng = np.random.default_rng(2401)
    bad_tf = 18
    a = 2 * (bad_tf * 196608 + 2656 + 1 * 2552)                       # symbols 1..3 of that TF (the null symbol and the phase reference stay)
    iq[a: a + 2 * 3 * 2552] = rng.integers(0, 256, 2 * 3 * 2552, dtype=np.uint8)
    want, _ = ol.or_replay(iq)
    flags = _good_flags(iq)
    bad_calls = [k for k, f in enumerate(flags) if f is False]
    assert len(bad_calls) == 1 and sum(1 for f in flags[:bad_calls[0]] if f) >= 14       # one bad TF, after lock and after the first frames
    assert len(want) >= 4 * (3 + 5)                                   # frames before the loss and after the second lock-in
    eng = dab.Engine(0)
    assert eng.decode([iq]) == len(want) and np.array_equal(eng.eti(0), want)
    assert eng.msc_deferred() == 9 == _expected_deferred(flags, [iq.size])[0]
    eng.close()
    seen = []
    for extra_calls in (0, 3):
        cut = (bad_calls[0] + 1 + extra_calls) * dab.CHUNK_BYTES
        st = dab.Stream(1, 0)
        got, deferred = [], []
        for seg in (iq[:cut], iq[cut:]):
            st.feed([seg])
            got.append(st.eti(0))
            deferred.append(st.msc_deferred())
        st.close()
        assert np.array_equal(np.concatenate(got), want), extra_calls
        assert deferred == _expected_deferred(flags, [cut, iq.size]), extra_calls
        seen.append(deferred)
    assert seen[0] == [9, 9] and seen[1][0] == 9 and 0 < seen[1][1] < 9, seen


def test_unequal_streams_and_one_too_short_to_lock():
    """(e) streams of unequal length in one batch, one of them shorter than ten TFs: all of it deferred, no frames, the others unaffected."""
    caps = [_capture(2501, 24), _capture(2502, 20, skip=3000), _capture(2503, 6), _capture(2504, 31, snr=5.0)]
    replays = [ol.or_replay(c) for c in caps]
    wants = [r[0] for r in replays]
    ntf = [sum(t.ok for t in r[1]) for r in replays]
    assert len(wants[2]) == 0 and 0 < ntf[2] < 10 and len(wants[0]) > len(wants[1]) > 0
    expect = [_expected_deferred(_good_flags(c), [c.size])[0] for c in caps]
    assert expect[:3] == [9, 9, ntf[2]]
    eng = dab.Engine(0)
    for demod_all in (False, True):
        eng.set_demod_all(demod_all)
        assert eng.decode(caps) == sum(len(w) for w in wants)
        assert eng.msc_deferred() == (0 if demod_all else sum(expect))
        assert [eng.eti_count(b) for b in range(4)] == [len(w) for w in wants]
        for b, w in enumerate(wants):
            assert np.array_equal(eng.eti(b), w), (demod_all, b)
    eng.set_demod_all(False)
    eng.decode(caps)
    fic, msc = eng.demapped_tf(2, ntf[2] - 1)                         # a TF of the stream that was deferred whole
    eng.set_demod_all(True)
    eng.decode(caps)
    fic_all, msc_all = eng.demapped_tf(2, ntf[2] - 1)
    assert np.array_equal(fic, fic_all) and np.array_equal(msc, msc_all)
    eng.close()
