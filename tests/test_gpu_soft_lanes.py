"""Soft decisions through the four-lane and the table-free two-lane decoder forms (vit_soft_lanes.hpp; opt-in: set_soft_lanes / soft_lanes=True).

  1. every code-word shape (64 UEP + 24 EEP) on identical values through the S3 seam, forms (four, four) and (two-plain, lane), against
     oracle/or_soft.c byte for byte, the form report naming the forced form on every frame; the four kinds of values (full, ties, zero, saturated)
     take turns ensemble by ensemble, as in test_gpu_soft.py: every shape meets one kind and every kind meets many shapes of every length class
     (what a kind exercises -- ties, erasures, metric growth -- is a property of the metric arithmetic, the same for every shape; what a shape
     exercises is its length and puncturing), which keeps each case to a fourth of the 88 x 4 decodes;
  2. the FIC in form four on values that do not decode: 4 blocks (one partial tile) through the S3 seam against or_fic_decode_soft; 64 blocks (one
     full tile) and 68 (a full tile and a partial one) from 16- and 17-TF captures at 5 dB against the forced lane form (the stage entry that takes
     injected FIC values carries hard bits only, so captures are the way to these counts; the lane form itself is held against the oracle by
     test_gpu_soft.py);
  3. values with about 5 % of -8 among them: forms four and two-plain equal the lane form byte for byte (the oracle is not the checker: what -8
     means is no contract of its);
  4. two streams x 24 TF at 5 dB: full and partial groups of 64 code words, several re-bases; Engine forced (four, four) against (lane, lane), and
     a session fed the same captures in three odd segments;
  5. the switch: off again, a forced four reports lane, same bytes; under AUTO the knob DABHIP_VIT_SOFT_FOUR_LANES picks four.
Integer arithmetic on both sides everywhere: no tolerance."""
import ctypes as C

import numpy as np
import pytest

import dabtools_amd as dab
import oracle_lib as ol
from test_gpu_parity_r2 import _profile_ensembles
from test_gpu_soft import _fic_values, _keep_mask, _msc_values

pytestmark = pytest.mark.gpu

KINDS = ["full", "ties", "zero", "saturated"]
EXTRA_TFS = 2                     # TFs of a capture that the front end spends on lock before it hands TFs on (the oracle's count, asserted in the test)


def _configure(ei, ens):
    cfg = dab.synth_preset(1, seed=700 + ei, cif_count0=245 + ei)
    cfg.nsub = len(ens)
    shapes = set()
    for k, (slform, idx, size, start) in enumerate(ens):
        cfg.sub[k].id = (7 * k + ei) % 64 if len(ens) <= 9 else k * 3
        cfg.sub[k].start_cu = start
        cfg.sub[k].slform = slform
        cfg.sub[k].uep_index = idx if slform == 0 else 0
        cfg.sub[k].eep_protlev = idx if slform == 1 else 0
        cfg.sub[k].size_cu = size
        shapes.add((slform, idx, size))
    return cfg, shapes


@pytest.fixture(scope="module")
def all_shapes():
    """[(FIC values, MSC values) x 16 TF, the oracle's 12 ETI frames] per ensemble; computed once, read by both form pairs.  Ensemble ei carries
    values of kind KINDS[ei % 4] (the rotation of test_gpu_soft.py, on purpose: see the module docstring)"""
    keep = _keep_mask()
    rng = np.random.default_rng(47)
    out, covered = [], set()
    for ei, ens in enumerate(_profile_ensembles()):
        cfg, shapes = _configure(ei, ens)
        covered |= shapes
        od = ol.SoftDab(ol.SOFT_Q4)
        tfs = []
        for t in range(16):
            fic, msc = _fic_values(cfg, t, keep), _msc_values(rng, KINDS[ei % len(KINDS)])
            od.process(fic, msc)
            tfs.append((fic, msc))
        want = np.array(od.frames)
        od.close()
        assert want.shape == (12, 6144), (ei, want.shape)
        out.append((tfs, want))
    assert len(covered) == 64 + 24
    assert len(out) >= len(KINDS)                            # every kind of values met at least once
    return out


@pytest.mark.parametrize("forms", [("four", "four"), ("two-plain", "lane")], ids=["four-four", "twoplain-lane"])
def test_every_code_word_shape_on_identical_values(forms, all_shapes):
    for ei, (tfs, want) in enumerate(all_shapes):
        d = dab.Dab(0, soft=True, soft_lanes=True, forms=forms)
        for fic, msc in tfs:
            d.fic[:] = fic
            d.msc[:] = msc
            ran = d.process_frame() > 0
            assert d.decoder_forms() == ({forms[0]} if ran else set(), {forms[1]}), (ei, forms)
        got = np.array(d.frames)
        d.close()
        assert got.shape == want.shape, (ei, got.shape)
        assert np.array_equal(got, want), "ensemble %d (%s values), forms %s: soft decode differs from the oracle" % (ei, KINDS[ei % len(KINDS)], forms)


def test_fic_four_lanes_one_partial_tile_against_the_oracle():
    O = ol.oracle()
    rng = np.random.default_rng(53)
    d = dab.Dab(0, soft=True, soft_lanes=True, forms=("four", "four"))
    for t, kind in enumerate(["full", "ties", "zero", "saturated", "full", "ties"]):
        fic = _msc_values(rng, kind)[:9216]
        want_fib = np.zeros((12, 32), np.uint8)
        want_ok = np.zeros(12, np.uint8)
        O.or_fic_decode_soft(ol._ptr(fic.astype(np.float32), C.c_float), ol.SOFT_Q4, ol._ptr(want_fib), ol._ptr(want_ok))
        d.fic[:] = fic
        d.msc[:] = 0
        d.process_frame()
        assert d.decoder_forms()[1] == {"four"}
        fibs, ok = d.last_fibs()
        assert np.array_equal(fibs, want_fib), (t, kind)
        assert np.array_equal(ok, want_ok), (t, kind)
    d.close()


@pytest.mark.parametrize("ntf", [16, 17])
def test_fic_four_lanes_full_and_partial_tiles_against_the_lane_form(ntf):
    """64 blocks (one full tile) and 68 (a full tile and a partial one): a capture at 5 dB of which ntf TFs are demodulated (the front end spends
    the first two on lock: the oracle's count, asserted here); checker of both counts: the forced lane form."""
    iq = dab.synth_generate(dab.synth_preset(1, seed=9400 + ntf, snr_db=5.0, cif_count0=77), ntf + EXTRA_TFS)
    assert ol.or_replay_soft(iq, ol.SOFT_Q4)[2] == ntf, "the capture demodulates to %d TFs = %d FIC blocks" % (ntf, 4 * ntf)
    out = {}
    for fic_form in ("lane", "four"):
        eng = dab.Engine(0)
        eng.set_soft(True)
        eng.set_soft_lanes(True)
        eng.set_decoder_forms("lane", fic_form)
        assert eng.decode([iq]) > 0
        assert eng.decoder_forms()[1] == {fic_form}
        out[fic_form] = eng.eti(0)
        eng.close()
    assert out["four"].shape == out["lane"].shape and out["four"].shape[0] > 0
    assert np.array_equal(out["four"], out["lane"])


def test_minus_eight_equals_the_lane_form():
    keep = _keep_mask()
    rng = np.random.default_rng(59)
    cfg, _ = _configure(0, _profile_ensembles()[0])
    tfs = []
    for t in range(20):
        # 16 TFs whose FIC decodes (lock takes ten good TFs in a row, the ring four more: 12 frames), -8 among its values all the same (a rate 1/3
        # code with a fortieth of its bits wrong); then four TFs of full-range FIC values that do not decode: lock is lost, the FIBs are compared
        fic = _fic_values(cfg, t, keep) if t < 16 else _msc_values(rng, "full")[:9216]
        msc = _msc_values(rng, "full")
        fic[rng.random(fic.size) < 0.05] = -8
        msc[rng.random(msc.size) < 0.05] = -8
        tfs.append((fic, msc))
    got = {}
    for forms in (("lane", "lane"), ("four", "four"), ("two-plain", "lane")):
        d = dab.Dab(0, soft=True, soft_lanes=True, forms=forms)
        fibs = []
        for fic, msc in tfs:
            d.fic[:] = fic
            d.msc[:] = msc
            ran = d.process_frame() > 0
            assert d.decoder_forms() == ({forms[0]} if ran else set(), {forms[1]}), forms
            fibs.append(np.concatenate([x.ravel() for x in d.last_fibs()]))
        got[forms] = (np.array(d.frames), np.array(fibs))
        d.close()
    want_frames, want_fibs = got[("lane", "lane")]
    assert want_frames.shape == (12, 6144) and want_fibs.shape[0] == 20
    for forms in (("four", "four"), ("two-plain", "lane")):
        assert np.array_equal(got[forms][0], want_frames), forms
        assert np.array_equal(got[forms][1], want_fibs), forms


@pytest.fixture(scope="module")
def two_streams():
    """Two whole captures of 24 TF: 22 demodulated TFs each, lock at the tenth, the ring four more: 36 ETI frames per stream, 72 code words per shape
    (a capture that starts inside a TF loses TFs to the front end and the pair would stay below 64)"""
    return [dab.synth_generate(dab.synth_preset(1, seed=9500 + b, snr_db=5.0, cif_count0=300 + 50 * b), 24) for b in range(2)]


def _engine_eti(streams, forms, soft_lanes=True):
    eng = dab.Engine(0)
    eng.set_soft(True)
    eng.set_soft_lanes(soft_lanes)
    eng.set_decoder_forms(*forms)
    assert eng.decode(streams) > 0
    report = eng.decoder_forms()
    eti = [eng.eti(b) for b in range(len(streams))]
    return eng, report, eti


def test_full_and_partial_groups_rebases_and_sessions(two_streams, monkeypatch):
    eng, report, want = _engine_eti(two_streams, ("lane", "lane"))
    eng.close()
    assert report == ({"lane"}, {"lane"})
    assert sum(e.shape[0] for e in want) > 64               # more than 64 code words of one shape: a full group and a partial one
    eng, report, got = _engine_eti(two_streams, ("four", "four"))
    eng.close()
    assert report == ({"four"}, {"four"})
    for b in range(2):
        assert np.array_equal(got[b], want[b]), b
    # a session (no forced forms there: the knobs put every launch in the four-lane form), the same captures in three odd segments
    for name, value in (("DABHIP_VIT_WAVE_MAX", "0"), ("DABHIP_FIC_WAVE_MAX", "0"), ("DABHIP_VIT_SOFT_FOUR_LANES", "1"), ("DABHIP_FIC_SOFT_FOUR_LANES", "1")):
        monkeypatch.setenv(name, value)
    ses = dab.Stream(2, soft=True)
    ses.set_soft_lanes(True)
    cuts = [0, 2345677, 6000001, None]
    frames = [[], []]
    for a, z in zip(cuts[:-1], cuts[1:]):
        ses.feed([iq[a:z] for iq in two_streams])
        for b in range(2):
            frames[b].append(ses.eti(b))
    ses.close()
    for b in range(2):
        assert np.array_equal(np.concatenate(frames[b]), want[b]), b


def test_the_switch(two_streams, monkeypatch):
    eng, report, want = _engine_eti(two_streams[:1], ("four", "four"))
    assert report == ({"four"}, {"four"})
    eng.set_soft_lanes(False)                                # off again: the same engine runs, and reports, the lane form
    assert eng.decode(two_streams[:1]) > 0
    assert eng.decoder_forms() == ({"lane"}, {"lane"})
    assert np.array_equal(eng.eti(0), want[0])
    eng.close()
    monkeypatch.setenv("DABHIP_VIT_SOFT_FOUR_LANES", "1")
    monkeypatch.setenv("DABHIP_VIT_WAVE_MAX", "0")
    eng = dab.Engine(0)
    eng.set_soft(True)
    eng.set_soft_lanes(True)
    assert eng.decode(two_streams[:1]) > 0
    assert eng.decoder_forms()[0] == {"four"}
    assert np.array_equal(eng.eti(0), want[0])
    eng.close()
