"""A stage entry leaves the trace of the decode before it alone.

The frame list on the device has a descriptor stride of its own (a stage entry's: its frames); trace() / trace_nco() index the host copy of the last
SCAN's descriptors with that scan's stride.  Before the two were one variable, a decision audit or stage_ofdm_fft over more frames than the decode had
calls made the next trace() read the descriptors with the wrong stride, and past their end.  Here: a decode of 2 streams x 12 calls, then both audits
and stage_ofdm_fft over 16 frames -- the traces stay bit-equal, a deferred TF's demapped values are refused (its frame list is gone), and the same
decode again gives the same frames.  Twice: at 12 calls (8 TFs: nothing locks, no frame is emitted -- the traces and the refusal are the point) and at
30 calls (20 TFs: lock at the tenth, nine deferred, ETI frames emitted by both streams), where the decode after the stage entries must reproduce real ETI bytes: the stage
entries rewrite the page-locked lists and the device frame list that a decode lays its frames out in."""
import numpy as np
import pytest

import dabtools_amd as dab
import oracle_lib as ol

pytestmark = pytest.mark.gpu


def _traces(eng):
    out = []
    for b in range(2):
        ints, ffs = eng.trace(b, 64)
        out.append((ints.copy(), ffs.copy(), eng.trace_nco(b, 64).copy()))
    return out


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for s, t in zip(a, b) for x, y in zip(s, t))


@pytest.mark.parametrize("NCALLS,NAUDIT,locks", [(12, 16, False), (30, 32, True)])
def test_trace_survives_stage_entries_over_more_frames_than_the_decode_had_calls(NCALLS, NAUDIT, locks):
    NBYTES = NCALLS * dab.CHUNK_BYTES                       # 8 / 20 transmission frames
    caps = [dab.synth_generate(dab.synth_preset(1, seed=3101 + b, cif_count0=77 * b, skip_samples=40000 * b), NBYTES // dab.TF_BYTES + 1)[:NBYTES] for b in range(2)]
    assert all(c.size == NBYTES for c in caps)
    frames = dab.synth_generate(dab.synth_preset(0, seed=3103, snr_db=9.0), NAUDIT)
    assert frames.size == NAUDIT * dab.TF_BYTES
    eng = dab.Engine(0)
    total = eng.decode(caps)
    want = _traces(eng)
    assert all(ints.shape == (NCALLS, 6) and ffs.shape == (NCALLS,) and nco.shape == (NCALLS,) for ints, ffs, nco in want)
    assert all(ints[:, 0].sum() >= 1 for ints, _, _ in want)            # frames were demodulated: the traces are not all zeros
    assert not np.array_equal(want[0][0], want[1][0])                    # and the two streams' differ (the second starts mid-frame): a wrong stride would show
    eti = [eng.eti(b) for b in range(2)]
    # 8 TFs: nothing locks, no frame; 20 TFs: lock at the tenth good TF, the frames of the TFs behind it -- the bytes compared below are real
    assert (total > 0 and all(e.shape[0] > 0 for e in eti)) if locks else total == 0
    for b in range(2):
        assert np.array_equal(eti[b], ol.or_replay(caps[b])[0]), b                 # (and they are the oracle's)
    deferred = eng.msc_deferred()
    assert deferred > 0                                                  # the leading TFs of both streams cannot be locked: their MSC part is deferred
    for what, run in (("audit", lambda: eng.decision_audit(frames=frames, guard=True)),
                      ("fused audit", lambda: eng.decision_audit(frames=frames, guard=True, fused=True)),
                      ("ofdm fft", lambda: eng.stage_ofdm_fft(frames, want_output=False))):
        run()
        assert _same(_traces(eng), want), what
    # the deferred TFs' samples are still there, but their frame list and descriptors are not: refused, not answered from another list
    with pytest.raises(dab.DabhipError):
        eng.demapped_tf(0, 0)
    assert eng.decode(caps) == total and eng.msc_deferred() == deferred
    assert _same(_traces(eng), want)
    for b in range(2):
        got = eng.eti(b)
        assert got.shape == eti[b].shape and np.array_equal(got, eti[b]), b
    eng.close()
