"""EEP sub-channels of every size through every decoder form, up to one that fills the CIF -- bit-exact everywhere, no tolerance.

The other decoder tests take each EEP level at n = 1, 2 and 8, and the longest code word any of them decodes is UEP 384 kbit/s: 9,222 trellis steps, 1,152
bytes per CIF.  The product accepts everything that fits the CIF and the ETI frame (layout_fault, control_plane.hpp): up to 43,782 steps (EEP 4-B at
n = 57, 5,472 bytes per CIF).  The shapes and their packing: tests/eep_sizes.py.  Which checker holds which range:

  up to 13,824 data bits (the REF ensembles)   the REAL back end (oracle/_ref) and the oracle, which must also agree with each other;
  above (the ORACLE ensembles)                 the oracle alone -- the reference's decoder is created for 768 * 18 bits (dab.c:29) and is past its own
                                               allocation there --, and, from captures, the payload the modulator sent (dabhip_synth_payload).

  1. hard decisions, the S3 seam of test_gpu_decoder_forms.py (structured FIC, random MSC bits, 16 TF -> 12 frames), in the five form pairs, the form
     report on every frame; one more pass of constant or periodic bits (all zeros, all ones, period 2, period 3: ties at every step) on each of the
     seven shapes that fill the CIF;
  2. soft decisions in the forms lane, wave and -- soft_lanes=True -- four and two-plain against oracle/or_soft.c on the four kinds of values of
     test_gpu_soft.py: each of the seven whole-CIF shapes on "saturated" AND on "ties" (metric growth and re-basing over 44 k steps is what a short code
     word cannot show), the other ensembles taking the kinds in turn;
  3. clean captures of one sub-channel through the whole path (Engine.decode: the default rule, lane and four forced): every frame == the oracle's
     replay, every sub-channel byte == the modulator's payload; one capture at 9 dB against the replay;
  4. the longest code word in full groups of 64: one capture handed to one decode 17 times;
  5. the largest sub-channel from a real decode into the MPEG-TS stage, on the device, against the modulator's words and ts_model.py;
  6. the S1 entry (Engine::viterbi_batch, the step-row viterbi_kernel) at the longest code word it takes, 49,152 bits = the 1,536 words of its zero
     table, against the oracle's or_viterbi, and its refusal one word above.

The real back end is REQUIRED as a checker wherever it can exist: where the reference's sources are present and oracle/_ref is missing all the same (a failed
build), the tests fail.  Only on a box with neither sources nor oracle/_ref is the hard test compared with the oracle alone, and says so by skipping at its
end, as test_gpu_decoder_forms.py does."""
import ctypes as C

import numpy as np
import pytest

import dabtools_amd as dab
import eep_sizes as sizes
import oracle_lib as ol
import test_gpu_decoder_forms as forms
import test_gpu_soft as soft
import test_gpu_ts as tts
import ts_model

pytestmark = pytest.mark.gpu

NTF = 16                           # hand-offs per ensemble: lock at the tenth, the 16-CIF ring four more -> 12 frames
KINDS = ["full", "ties", "zero", "saturated"]
TIE_KINDS = ["zeros", "ones", "period2", "period3"]          # the tie-heavy CIFs of test_gpu_decoder_forms.py, without its "random-cif"


def _real_back_end():
    """oracle/_ref's back end; None only where it cannot exist (no sources of the reference on this box, and none built elsewhere and brought along)"""
    R = ol.ref()
    assert R is not None or not ol.ref_sources_present(), "the reference's sources are here but oracle/_ref/libdabref.so is not: its build failed, the REF checker is lost"
    return R


def _cases():
    """[(checker, ensemble index for seeds and SubChIds, ensemble)]: the REF ensembles, then the ORACLE ones (the first seven fill the CIF)."""
    ref, oracle = sizes.ensembles()
    return [("REF", 100 + i, ens) for i, ens in enumerate(ref)] + [("ORACLE", 200 + k, ens) for k, ens in enumerate(oracle)]


def _whole_cif(ens):
    return ens[-1][:3] in sizes.WHOLE_CIF_ITEMS


def _what(ens):
    return " + ".join(sizes.name(it) for it in ens)


def _oracle_and_real(checker, inputs):
    """The oracle's ETI frames of the hand-offs and -- REF ensembles only: beyond 13,824 bits its decoder is past its allocation -- the real back end's."""
    R, O = _real_back_end(), ol.oracle()
    frames_or = []
    CB = C.CFUNCTYPE(None, C.POINTER(C.c_uint8), C.c_void_p)
    cb = CB(lambda p, u: frames_or.append(np.ctypeslib.as_array(p, (6144,)).copy()))
    od = O.or_dab_new(C.cast(cb, C.c_void_p), None)
    H = R.refh_new() if (R is not None and checker == "REF") else None
    for fic, msc in inputs:
        C.memmove(O.or_dab_tf_fic(od), ol._ptr(fic), fic.size)
        C.memmove(O.or_dab_tf_msc(od), ol._ptr(msc), msc.size)
        O.or_dab_process_frame(od)
        if H is not None:
            C.memmove(R.refh_tf_fic(H), ol._ptr(fic), fic.size)
            C.memmove(R.refh_tf_msc(H), ol._ptr(msc), msc.size)
            R.refh_process(H)
    O.or_dab_free(od)
    real = None
    if H is not None:
        n = R.refh_neti(H)
        real = np.ctypeslib.as_array(R.refh_eti(H), (n, 6144)).copy()
    return np.array(frames_or), real


# ---- 1. hard decisions ------------------------------------------------------------------------------------------------------------
def _hard_runs():
    """(pass, checker, ei, ensemble): random bits on everything, the tie-heavy pass on the seven whole-CIF shapes"""
    cases = _cases()
    return [(0,) + c for c in cases] + [(1,) + c for c in cases if _whole_cif(c[2])]


def _tie_kind(ens):
    """The pass-1 pattern of a whole-CIF ensemble: by its place among the seven, so that each gets a tie-heavy one and all four kinds are met"""
    return TIE_KINDS[sizes.WHOLE_CIF_ITEMS.index(ens[-1][:3]) % len(TIE_KINDS)]


def _seam_inputs(pass_, ei, ens, keep):
    """The 16 (FIC, MSC) hand-offs of an ensemble: structured FIC (the multiplex is found); MSC random (pass 0) or the same tie-heavy CIF in every CIF of
    every TF (pass 1: the time de-interleaver leaves such a pattern as it is)."""
    O = ol.oracle()
    cfg = sizes.configure(ei, ens)
    rng = np.random.default_rng(1000 * pass_ + ei + 31)
    if pass_ == 1:
        n = np.arange(55296)
        cif = {"zeros": np.zeros(55296, np.uint8), "ones": np.ones(55296, np.uint8), "period2": (n % 2).astype(np.uint8),
               "period3": (n % 3 == 0).astype(np.uint8)}[_tie_kind(ens)]
    for t in range(NTF):
        fic = np.zeros(9216, np.uint8)
        for q in range(4):
            f = dab.synth_fibs(cfg, 4 * t + q).copy()
            O.or_descramble(ol._ptr(f), 96)
            fic[2304 * q:2304 * (q + 1)] = ol.or_encode(f)[keep]
        yield fic, (rng.integers(0, 2, 221184, dtype=np.uint8) if pass_ == 0 else np.tile(cif, 4))


def _hard_reference():
    keep = forms._keep()
    out = {}
    for pass_, checker, ei, ens in _hard_runs():
        frames_or, real = _oracle_and_real(checker, _seam_inputs(pass_, ei, ens, keep))
        assert frames_or.shape == (12, 6144), (_what(ens), frames_or.shape)
        if real is not None:                               # the two checkers agree with each other
            assert real.shape == (12, 6144) and np.array_equal(real, frames_or), "REF and ORACLE differ on " + _what(ens)
        out[pass_, ei] = (frames_or, real)
    return keep, out


@pytest.fixture(scope="module")
def hard_reference():
    return _hard_reference()


@pytest.mark.parametrize("msc,fic", forms.FORM_PAIRS)
def test_hard_decisions_every_size_in_every_form(msc, fic, hard_reference):
    keep, want = hard_reference
    runs = _hard_runs()
    ties = [_tie_kind(r[3]) for r in runs if r[0] == 1]
    assert len(ties) == 7 and set(ties) == set(TIE_KINDS) and "random-cif" not in ties          # each whole-CIF shape on a tie-heavy pattern, never a random one
    wrong, covered = [], set()
    for pass_, checker, ei, ens in runs:
        covered.update(it[:3] for it in ens)
        d = dab.Dab(0, forms=(msc, fic))
        for fic_bits, msc_bits in _seam_inputs(pass_, ei, ens, keep):
            d.fic[:] = fic_bits
            d.msc[:] = msc_bits
            r = d.process_frame()
            forms._assert_report(d, msc, fic, msc_ran=r > 0)
        got = np.array(d.frames)
        assert d.status == 0, _what(ens)
        d.close()
        frames_or, real = want[pass_, ei]
        what = "%s/%s, %s MSC, %s" % (msc, fic, "random" if pass_ == 0 else _tie_kind(ens), _what(ens))
        assert got.shape == (12, 6144), (what, got.shape)
        assert (got[0][5] & 0x7f) == len(ens), what
        # (every ensemble is decoded before the verdict, so that a failure names all the shapes it concerns)
        if not np.array_equal(got, frames_or):
            wrong.append(what + ": differs from the oracle")
        if checker == "REF" and real is not None and not np.array_equal(got, real):
            wrong.append(what + ": differs from the real reference")
    assert not wrong, "\n".join(wrong)
    assert covered >= set(sizes.REF_ITEMS) | set(sizes.ORACLE_ITEMS)
    if _real_back_end() is None:
        pytest.skip("compared with the oracle only: neither the reference's sources nor oracle/_ref on this box")


# ---- 2. soft decisions ------------------------------------------------------------------------------------------------------------
def _soft_runs():
    """(ei, ensemble, kind of values): the seven whole-CIF shapes on saturated values and on ties, the others taking the four kinds in turn"""
    runs, turn = [], 0
    for _, ei, ens in _cases():
        if _whole_cif(ens):
            runs += [(ei, ens, "saturated"), (ei, ens, "ties")]
        else:
            runs.append((ei, ens, KINDS[turn % len(KINDS)]))
            turn += 1
    return runs


def _soft_reference():
    """[(what, len(ensemble), the 16 (FIC values, MSC values), the oracle's 12 frames)], computed once for the four forms"""
    keep = soft._keep_mask()
    out = []
    for ei, ens, kind in _soft_runs():
        cfg = sizes.configure(ei, ens)
        rng = np.random.default_rng(7000 + 10 * ei + KINDS.index(kind))
        od = ol.SoftDab(ol.SOFT_Q4)
        tfs = []
        for t in range(NTF):
            fic, msc = soft._fic_values(cfg, t, keep), soft._msc_values(rng, kind)
            od.process(fic, msc)
            tfs.append((fic, msc))
        want = np.array(od.frames)
        od.close()
        assert want.shape == (12, 6144), (_what(ens), kind, want.shape)
        out.append(("%s values, %s" % (kind, _what(ens)), len(ens), tfs, want))
    return out


@pytest.fixture(scope="module")
def soft_reference():
    return _soft_reference()


def test_the_soft_runs_give_every_whole_cif_shape_saturated_values_and_ties():
    runs = _soft_runs()
    for it in sizes.WHOLE_CIF_ITEMS:
        assert {kind for _, ens, kind in runs if ens[-1][:3] == it} == {"saturated", "ties"}, sizes.name(it)
    assert {kind for _, _, kind in runs} == set(KINDS)
    assert {it[:3] for _, ens, _ in runs for it in ens} >= set(sizes.REF_ITEMS) | set(sizes.ORACLE_ITEMS)


@pytest.mark.parametrize("soft_lanes,pair", [(False, ("lane", "lane")), (False, ("wave", "wave")), (True, ("four", "four")), (True, ("two-plain", "lane"))],
                         ids=["lane", "wave", "four", "twoplain"])
def test_soft_decisions_every_size(soft_lanes, pair, soft_reference):
    wrong = []
    for what, nsub, tfs, want in soft_reference:
        d = dab.Dab(0, soft=True, soft_lanes=soft_lanes, forms=pair)
        for fic, msc in tfs:
            d.fic[:] = fic
            d.msc[:] = msc
            ran = d.process_frame() > 0
            assert d.decoder_forms() == ({pair[0]} if ran else set(), {pair[1]}), (what, pair)
        got = np.array(d.frames)
        d.close()
        assert got.shape == want.shape and (got[0][5] & 0x7f) == nsub, (what, got.shape)
        if not np.array_equal(got, want):
            wrong.append("%s, forms %s: soft decode differs from the oracle" % (what, pair))
    assert not wrong, "\n".join(wrong)


# ---- 3. by construction, through the whole path -------------------------------------------------------------------------------------
CAPTURE_TF = 18                    # the front end spends two TFs on lock before it hands TFs on: 16 reach the back end, 12 frames come out
CAPTURES = {"4-A n=216": (3, 216, 0), "4-B n=57": (7, 57, 9), "4-A n=171": (3, 171, 100), "3-A n=9": (2, 9, 400)}        # level, n, start_cu


def _one_subchannel_cfg(key, seed, **kw):
    level, n, start = CAPTURES[key]
    cfg = dab.synth_preset(1, seed=seed, **kw)
    cfg.nsub = 1
    s = cfg.sub[0]
    s.id, s.start_cu, s.slform, s.uep_index, s.eep_protlev, s.size_cu = 5, start, 1, 0, level, sizes.CU_PER_UNIT[level] * n
    sizes.check_layout([(1, level, s.size_cu, start)])
    return cfg


def _payload_errors(cfg, frames, ntf):
    """Wrong bits of the one sub-channel of every frame against what the modulator sent in that logical CIF, and the bits compared"""
    cifs = tts._cifs_of(cfg, frames, ntf)
    per = dab.synth_payload(cfg, 0, 0).size
    assert per == sizes.bytes_per_cif(sizes.item(cfg.sub[0].eep_protlev, cfg.sub[0].size_cu // sizes.CU_PER_UNIT[cfg.sub[0].eep_protlev]))
    wrong = 0
    for f, cif in zip(frames, cifs):
        assert (f[5] & 0x7f) == 1
        data = f[12 + 4 + 96:][:per]
        wrong += int(np.unpackbits(data ^ dab.synth_payload(cfg, cif, 0)).sum())
    return wrong, 8 * per * len(frames)


def _captures():
    """{name: (cfg, IQ bytes, the oracle's replay)}: the four clean ones, whose replay is held against the payload here, and 4-B n = 57 at 9 dB"""
    out = {}
    for i, key in enumerate(CAPTURES):
        cfg = _one_subchannel_cfg(key, 9700 + i, cif_count0=245 + 1000 * i)
        iq = dab.synth_generate(cfg, CAPTURE_TF)
        want, _ = ol.or_replay(iq)
        assert want.shape == (12, 6144), (key, want.shape)
        wrong, bits = _payload_errors(cfg, list(want), CAPTURE_TF)
        assert wrong == 0 and bits > 0, (key, wrong, bits)
        out[key] = (cfg, iq, want)
    cfg = _one_subchannel_cfg("4-B n=57", 9710, cif_count0=77, snr_db=9.0)
    iq = dab.synth_generate(cfg, CAPTURE_TF)
    out["4-B n=57 at 9 dB"] = (cfg, iq, ol.or_replay(iq)[0])
    return out


@pytest.fixture(scope="module")
def captures():
    return _captures()


ENGINE_FORMS = [("auto", "auto"), ("lane", "lane"), ("four", "four")]


@pytest.mark.parametrize("key", list(CAPTURES) + ["4-B n=57 at 9 dB"])
def test_one_subchannel_captures_equal_the_replay_and_the_payload(key, captures):
    cfg, iq, want = captures[key]
    assert want.shape[0] > 0
    for msc, fic in ENGINE_FORMS:
        eng = dab.Engine(0)
        eng.set_decoder_forms(msc=msc, fic=fic)
        total = eng.decode([iq])
        if msc == "auto":
            assert eng.decoder_forms() == ({"wave"}, {"wave"})              # a handful of code words: the default rule's low-latency form
        else:
            forms._assert_report(eng, msc, fic)
        got = eng.eti(0)
        assert eng.stream_status(0) == 0
        eng.close()
        assert total == want.shape[0] and got.shape == want.shape, (key, msc, got.shape)
        assert np.array_equal(got, want), "%s, %s form: differs from the oracle's replay" % (key, msc)
        if key in CAPTURES:
            assert _payload_errors(cfg, list(got), CAPTURE_TF)[0] == 0, (key, msc)


# ---- 4. full groups at the longest length ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("msc,fic", [("lane", "lane"), ("auto", "auto")])
def test_full_groups_of_the_longest_code_word(msc, fic, captures):
    """17 streams of 12 frames share the one code-word plan: 204 code words of 43,782 steps = three full groups of 64 and one of 12."""
    cfg, iq, want = captures["4-B n=57"]
    nstreams = 17
    eng = dab.Engine(0)
    eng.set_decoder_forms(msc=msc, fic=fic)
    assert eng.decode([iq] * nstreams) == nstreams * want.shape[0]
    steps, _ = eng.msc_plan()
    ncw = nstreams * want.shape[0]
    assert ncw > 64 and steps.tolist() == [43782] * -(-ncw // 64), steps
    assert eng.decoder_forms()[0] == {"lane" if msc == "lane" else "wave"}
    first = eng.eti(0)
    assert np.array_equal(first, want), "stream 0 differs from the oracle"
    for b in range(1, nstreams):
        assert np.array_equal(eng.eti(b), first), b
    eng.close()


# ---- 5. the largest sub-channel into the TS stage from a real decode ------------------------------------------------------------------
def test_whole_cif_subchannel_from_the_decoder_into_the_ts_stage():
    cfg = _one_subchannel_cfg("4-A n=216", 9720, cif_count0=4321)
    cfg.ts_slots = 1
    cfg.ts_phase = 1234
    scid = cfg.sub[0].id
    iq = dab.synth_generate(cfg, CAPTURE_TF)
    want_frames, _ = ol.or_replay(iq)
    assert want_frames.shape == (12, 6144)
    eng = dab.Engine(0)
    assert eng.decode([iq]) == 12
    assert np.array_equal(eng.eti(0), want_frames)
    ptr, total = eng.eti_device_ptr()
    assert total == 12
    ts = dab.Ts(1, [scid])
    assert ts.push((ptr, [12])) > 0
    # the modulator's own words
    pos, data = tts._truth(cfg, 0, tts._cifs_of(cfg, want_frames, CAPTURE_TF))
    recs, got = ts.records(0, 0), ts.data(0, 0)
    st = dict(zip(dab.TS_STATS, ts.stats(0, 0)))
    assert len(pos) > 250 and recs["pos"].tolist() == pos and (got == data).all(), st
    assert st["packets"] == len(pos) and st["bytes_skipped"] == pos[0] and sum(ts.stats(0, 0)[[1, 2, 4, 5, 6]]) == 0, st
    # the model on the oracle's frames
    want, stats = tts._expect([list(want_frames)], [scid])
    assert len(want[0, 0][0]) == len(pos) and dict(zip(ts_model.STATS, stats[0, 0]))["sync_losses"] == 0
    tts._assert_equal(ts, {(0, 0): tts._gpu_lane(ts, 0, 0)}, want, stats, "4-A n=216 through the decoder")
    ts.close()
    eng.close()


# ---- 6. the S1 entry at the end of its zero table ---------------------------------------------------------------------------------------
S1_MAX_BITS = 32 * 1536            # kMaxCodewordWords words of 32 data bits (dab_tables.hpp)


def test_s1_entry_at_its_longest_code_word_and_the_refusal_above():
    """Three code words of 49,152 bits (one partial group): noisy with erasures, all erased (every compare a tie: all-zero data), and the half-erased
    alternating pattern of test_viterbi_all_erased_and_ties; the step-row kernel's decisions == the oracle's scalar decoder.  One word more is refused."""
    assert S1_MAX_BITS == 8 * dab.ETI_BYTES
    import test_gpu_parity as parity
    per = 4 * (S1_MAX_BITS + 6)
    noisy, _ = parity._noisy_codewords(np.random.default_rng(61), S1_MAX_BITS, 1, 0.3, 0.08)
    erased = np.full(per, 128, np.uint8)
    ties = erased.copy()
    ties[::2] = 127
    ties[1::8] = 129
    sym = np.concatenate([noisy, erased, ties])
    got = dab.viterbi(sym, S1_MAX_BITS, 3)
    assert got.shape == (3, S1_MAX_BITS // 8) and not got[1].any()
    for i in range(3):
        assert np.array_equal(got[i], ol.or_viterbi(sym[i * per:(i + 1) * per], S1_MAX_BITS)), i
    with pytest.raises(dab.DabhipError, match="code word too long"):
        dab.viterbi(np.full(4 * (S1_MAX_BITS + 32 + 6), 128, np.uint8), S1_MAX_BITS + 32)
    assert not dab.viterbi(erased, S1_MAX_BITS, 1).any()              # the entry goes on working after the refusal
