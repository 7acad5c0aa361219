"""The two forms of the channel decoder on the same input (hard decisions = reference semantics, viterbi.c:352-451):
one wave per code word (k_vitwave.hip, small batches: the single live ensemble of dab2eti.c:60-115), one lane per code word
(viterbi_fused_kernel, the batch form) and four lanes per code word (vit_four_lanes.hpp) must produce identical ETI bytes -- and the oracle's."""
import numpy as np
import pytest

import dabtools_amd as dab
import oracle_lib as ol

pytestmark = pytest.mark.gpu


def _streams():
    out = []
    for seed, skip, snr, preset in ((501, 0, 1000.0, 0), (502, 41000, 9.0, 0), (503, 0, 7.5, 1), (504, 150000, 1000.0, 1)):
        cfg = dab.synth_preset(preset, seed=seed, cif_count0=4980 + seed % 7, skip_samples=skip, snr_db=snr)
        out.append(dab.synth_generate(cfg, 21))
    return out


def test_wave_form_equals_lane_form_equals_oracle():
    """4 streams x 21 TF (about 100 groups of 64 code words): the default rule would send this batch to the four-lane form unless the
    wave form took it, so each form is pinned (Engine.set_decoder_forms) and the report confirms the kernel that ran."""
    streams = _streams()
    want = [ol.or_replay(iq)[0] for iq in streams]
    got = {}
    for form in ("wave", "lane", "four"):
        eng = dab.Engine(0)
        eng.set_decoder_forms(msc=form, fic=form)
        assert eng.decode(streams) == sum(w.shape[0] for w in want)
        assert eng.decoder_forms() == ({form}, {form})
        got[form] = [eng.eti(b) for b in range(len(streams))]
        eng.close()
    for b in range(len(streams)):
        assert want[b].shape[0] > 0
        for form in got:
            assert np.array_equal(got[form][b], want[b]), "stream %d: %s form differs from the oracle" % (b, form)


def test_wave_form_on_every_code_word_length_against_the_real_reference():
    """All 64 UEP + 24 EEP shapes, random MSC bits (what comes out is the decoder's tie rule and metric, nothing else), through the S3 seam
    with the wave form forced for every size (the 384 kbit/s code word, 9222 steps, runs two waves to a workgroup)."""
    import test_gpu_parity_r2 as r2
    r2.test_all_uep_and_eep_profiles_through_process_frame(forms=("wave", "wave"))
