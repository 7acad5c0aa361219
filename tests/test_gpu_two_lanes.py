"""The decoder with two and with four lanes per code word (vit_two_lanes.hpp, vit_four_lanes.hpp: mid-size batches, hard decisions) against the lane form and
the oracle: the same bytes.  (The whole suite also runs with every lane-form decode forced through them: tools/gpu/two_lanes.sh, four_lanes.sh STAGE=suite.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# form -> (MSC, FIC) decoder forms: 0 = one lane per code word, 1 = two lanes (vit_two_lanes.hpp), 2 = two lanes without tables,
# 4 = four lanes (vit_four_lanes.hpp); the FIC follows the lane form (0) or the four-lane form (4), and takes the lane form beside the two-lane ones
FORMS = {0: ("lane", "lane"), 1: ("two", "lane"), 2: ("two-plain", "lane"), 4: ("four", "four")}


def _engine(dab, form):
    eng = dab.Engine(0)
    eng.set_decoder_forms(*FORMS[form])
    return eng


def _decode(eng, caps, form):
    n = eng.decode(caps)
    assert eng.decoder_forms() == tuple({f} for f in FORMS[form]), form
    return n


@pytest.mark.parametrize("preset,streams,tfs", [(0, 10, 26), (1, 7, 21)])
def test_two_lanes_per_code_word_decode_what_the_lane_form_and_the_oracle_decode(preset, streams, tfs):
    import dabtools_amd as dab
    import oracle_lib as ol
    # noisy enough that the decoders correct errors all the time and metrics tie (9 .. 13 dB, hard decisions), every stream its own payload and offset
    caps = [dab.synth_generate(dab.synth_preset(preset, seed=7100 + 13 * b + preset, cif_count0=37 * b, skip_samples=1000 * b, snr_db=9.0 + (b % 5)), tfs) for b in range(streams)]
    out = {}
    for mode in (0, 1, 2, 4):
        eng = _engine(dab, mode)
        n = _decode(eng, caps, mode)
        out[mode] = [eng.eti(b) for b in range(streams)]
        assert n == sum(x.shape[0] for x in out[mode]) and n > 0
        eng.close()
    for mode in (1, 2, 4):
        for b in range(streams):
            assert out[0][b].shape == out[mode][b].shape and np.array_equal(out[0][b], out[mode][b]), (mode, b)
    for b in (0, streams - 1):
        want, _ = ol.or_replay(caps[b], cap_frames=4 * tfs)
        assert want.shape[0] > 0 and np.array_equal(out[4][b], want) and np.array_equal(out[1][b], want), b


def test_the_default_rule_takes_two_lanes_for_a_mid_size_batch_and_the_bytes_do_not_depend_on_it():
    import dabtools_amd as dab
    # 16 streams x 24 TF of the 12-sub-channel multiplex = 6,912 code words in 9 x 4 x 16 frames: above the wave form's range only with the knob; the default
    # engine takes whatever its rules say -- the bytes must be those of the forced forms
    caps = [dab.synth_generate(dab.synth_preset(0, seed=7300 + b, snr_db=11.0), 24) for b in range(16)]
    ref = None
    for mode in (None, 0, 1, 4):
        if mode is None:
            eng = dab.Engine(0)
            eng.decode(caps)
        else:
            eng = _engine(dab, mode)
            _decode(eng, caps, mode)
        got = np.concatenate([eng.eti(b) for b in range(16)])
        eng.close()
        if ref is None:
            ref = got
        assert got.shape == ref.shape and np.array_equal(got, ref), mode
