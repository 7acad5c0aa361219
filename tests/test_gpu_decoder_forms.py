"""Every form of the hard-decision Viterbi decoder against the reference (viterbi.c:352-451), each one pinned by
dabhip_engine_set_decoder_forms / dabhip_dab_set_decoder_forms and confirmed by the decoder-form report after every decode:

  MSC: wave (k_vitwave.hip), lane (viterbi_fused_kernel<1>), two (vit_two_lanes.hpp), two-plain and four (vit_four_lanes.hpp)
  FIC: wave, lane, four

(a) the S3 seam on all 64 UEP + 24 EEP code-word shapes, random and tie-heavy MSC bits, against the REAL back end (oracle/_ref) and the oracle:
    one TF per call, so every group of code words is partial;
(b) the batch engine on three multiplexes at 5 .. 9 dB (the decoders correct errors all the time), full groups of 64 code words, against the
    oracle's replay of every stream, per-call traces included;
(c) the FIC decoder at its tile edges (1, 16, 17, 512, 513 frames = 4 .. 2052 blocks in tiles of 64) on clean, correctable, uncorrectable and
    random blocks, against the oracle's and (for a sample) the REAL fic_decode;
(d) the default rule picks the forms engine.hpp documents for the batch sizes README and DESIGN quote;
(e) a multi-lane form asked of a soft-decision engine runs, and reports, the lane form.

A launch split into several slices (Engine::launch_decode_batch's slice_start; by default only past 24 GiB of survivor records per launch) is held by
tests/test_gpu_launch_splits.py, which lowers the row limit until every form runs in many slices."""
import ctypes as C

import numpy as np
import pytest

import dabtools_amd as dab
import oracle_lib as ol
import test_gpu_parity_r2 as r2

pytestmark = pytest.mark.gpu

# (MSC form, FIC form) pairs: every form of each decoder at least once
FORM_PAIRS = [("wave", "wave"), ("lane", "lane"), ("two", "four"), ("two-plain", "lane"), ("four", "four")]
MSC_FORMS = ["wave", "lane", "two", "two-plain", "four"]
FIC_OF = dict(FORM_PAIRS)


def _assert_report(obj, msc, fic, msc_ran=True, fic_ran=True):
    """The report after one decode: exactly the forced form ran (bit 1 << form), or nothing where no such launch was due."""
    m, f = obj.decoder_forms(masks=True)
    assert m == ((1 << dab.FORMS[msc]) if msc_ran else 0), ("MSC forms that ran", m, msc)
    assert f == ((1 << dab.FORMS[fic]) if fic_ran else 0), ("FIC forms that ran", f, fic)


# ---- (a) every code-word shape through the S3 seam -------------------------------------------------------------------------------
STRUCTURED = ["zeros", "ones", "period2", "period3", "random-cif"]


def _keep():
    dep = np.zeros(3096, np.uint8)
    ol.oracle().or_fic_depuncture(ol._ptr(dep), ol._ptr(np.zeros(2304, np.uint8)))
    return dep != 128


def _profile_cfg(ei, ens):
    cfg = dab.synth_preset(1, seed=900 + ei, cif_count0=240 + ei)      # (as test_gpu_parity_r2: the CIF counter wraps 249 -> 0 inside the run)
    cfg.nsub = len(ens)
    for k, (slform, idx, size, start) in enumerate(ens):
        cfg.sub[k].id = (7 * k + ei) % 64 if len(ens) <= 9 else k * 3
        cfg.sub[k].start_cu = start
        cfg.sub[k].slform = slform
        cfg.sub[k].uep_index = idx if slform == 0 else 0
        cfg.sub[k].eep_protlev = idx if slform == 1 else 0
        cfg.sub[k].size_cu = size
    return cfg


def _seam_inputs(pass_, ei, ens, keep):
    """The 16 (FIC, MSC) hand-offs of ensemble ei: structured FIC (the multiplex is found); MSC random (pass 0) or the same tie-heavy
    CIF in every CIF of every TF (pass 1: the time de-interleaver leaves the pattern as it is)."""
    O = ol.oracle()
    cfg = _profile_cfg(ei, ens)
    rng = np.random.default_rng(1000 * pass_ + ei + 31)
    kind = STRUCTURED[ei % len(STRUCTURED)]
    cif = {"zeros": np.zeros(55296, np.uint8), "ones": np.ones(55296, np.uint8), "period2": (np.arange(55296) % 2).astype(np.uint8),
           "period3": (np.arange(55296) % 3 == 0).astype(np.uint8), "random-cif": rng.integers(0, 2, 55296, dtype=np.uint8)}[kind]
    for t in range(16):
        fic = np.zeros(9216, np.uint8)
        for q in range(4):
            f = dab.synth_fibs(cfg, 4 * t + q).copy()
            O.or_descramble(ol._ptr(f), 96)
            fic[2304 * q:2304 * (q + 1)] = ol.or_encode(f)[keep]
        msc = rng.integers(0, 2, 221184, dtype=np.uint8) if pass_ == 0 else np.tile(cif, 4)
        yield fic, msc


@pytest.fixture(scope="module")
def seam_reference():
    """Per (pass, ensemble): the oracle's ETI frames and the REAL back end's (None without oracle/_ref) -- computed once, reused for every form."""
    R, O = ol.ref(), ol.oracle()
    keep = _keep()
    ensembles = r2._profile_ensembles()
    out = {}
    for pass_ in (0, 1):
        for ei, ens in enumerate(ensembles):
            frames_or = []
            CB = C.CFUNCTYPE(None, C.POINTER(C.c_uint8), C.c_void_p)
            cb = CB(lambda p, u: frames_or.append(np.ctypeslib.as_array(p, (6144,)).copy()))
            od = O.or_dab_new(C.cast(cb, C.c_void_p), None)
            H = R.refh_new() if R is not None else None
            for fic, msc in _seam_inputs(pass_, ei, ens, keep):
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
            out[(pass_, ei)] = (np.array(frames_or), real)
    return ensembles, keep, out


@pytest.mark.parametrize("msc,fic", FORM_PAIRS)
def test_every_code_word_shape_in_every_form_against_the_real_back_end(msc, fic, seam_reference):
    ensembles, keep, want = seam_reference
    covered = set()
    for pass_ in (0, 1):
        for ei, ens in enumerate(ensembles):
            covered.update((s, i, z) for s, i, z, _ in ens)
            d = dab.Dab(0, forms=(msc, fic))
            for fic_bits, msc_bits in _seam_inputs(pass_, ei, ens, keep):
                d.fic[:] = fic_bits
                d.msc[:] = msc_bits
                r = d.process_frame()
                _assert_report(d, msc, fic, msc_ran=r > 0)
            got = np.array(d.frames)
            d.close()
            frames_or, real = want[(pass_, ei)]
            what = "%s/%s, %s MSC, ensemble %d" % (msc, fic, "random" if pass_ == 0 else STRUCTURED[ei % len(STRUCTURED)], ei)
            assert got.shape == (12, 6144), (what, got.shape)
            assert (got[0][5] & 0x7f) == len(ens), what
            assert np.array_equal(got, frames_or), what + ": differs from the oracle"
            if real is not None:
                assert np.array_equal(got, real), what + ": differs from the real reference"
    assert len(covered) == 64 + 24
    if ol.ref() is None:
        pytest.skip("compared with the oracle only: oracle/_ref not built on this box")


# ---- (b) full groups through the batch engine --------------------------------------------------------------------------------------
def _dense_cfg(seed, snr):
    """The 20-sub-channel multiplex of test_gpu_parity.test_engine_many_subchannels_and_uep_eep_mix."""
    cfg = dab.synth_preset(0, seed=seed, snr_db=snr, cif_count0=(31 * seed) % 5000)
    cfg.nsub = 0
    cu = 0
    uep_cu = [16, 21, 24, 29, 35, 24, 29, 35, 42, 52, 29, 35, 42, 52, 32, 42, 48, 58, 70, 40]
    for slform, idx, size in [(0, i, 0) for i in (0, 4, 5, 9, 14, 18)] + \
            [(1, lev, size) for lev, size in ((0, 12), (1, 8), (2, 6), (3, 4), (4, 27), (5, 21), (6, 18), (7, 15), (0, 96), (3, 64), (1, 16), (2, 12), (3, 8), (7, 30))]:
        k = cfg.nsub
        cfg.sub[k].id = 3 * k + 1
        cfg.sub[k].start_cu = cu
        cfg.sub[k].slform = slform
        if slform == 0:
            cfg.sub[k].uep_index = idx
            cu += uep_cu[idx]
        else:
            cfg.sub[k].eep_protlev = idx
            cfg.sub[k].size_cu = size
            cu += size
        cfg.nsub += 1
    assert cfg.nsub == 20 and cu <= 864
    return cfg


BATCH_TF = 32


@pytest.fixture(scope="module")
def noisy_batch():
    """24 streams x 32 TF at 5, 7 and 9 dB: 8 of each multiplex (preset 0: 12 sub-channels, preset 1: 4, the dense one: 20), and the
    oracle's replay of each stream, once.  One after the other: the oracle's front end keeps static scratch buffers (or_frontend.c), so
    replays on several threads of one process corrupt one another."""
    caps, kinds = [], []
    for b in range(24):
        kind, snr = b % 3, (5.0, 7.0, 9.0)[(b // 3) % 3]
        seed = 8100 + b
        cfg = _dense_cfg(seed, snr) if kind == 2 else dab.synth_preset(kind, seed=seed, snr_db=snr, cif_count0=(97 * b) % 5000, skip_samples=1700 * b)
        caps.append(dab.synth_generate(cfg, BATCH_TF))
        kinds.append((kind, cfg.nsub))
    want = [ol.or_replay(iq) for iq in caps]
    return caps, kinds, want


def test_full_groups_in_every_msc_form_against_the_oracle(noisy_batch):
    caps, kinds, want = noisy_batch
    # full groups: the streams of one multiplex share its code-word plans (same shapes, same places in the frame), so a plan holds one code
    # word per ETI frame of all of them -- groups of exactly 64 wherever that is >= 64
    per_kind = {}
    for (kind, nsub), (eti, _) in zip(kinds, want):
        per_kind[kind] = per_kind.get(kind, 0) + eti.shape[0]
    assert len(per_kind) == 3 and all(n >= 64 for n in per_kind.values()), per_kind
    got = {}
    for msc in MSC_FORMS:
        eng = dab.Engine(0)
        eng.set_decoder_forms(msc=msc, fic=FIC_OF[msc])
        total = eng.decode(caps)
        _assert_report(eng, msc, FIC_OF[msc])
        assert total == sum(w[0].shape[0] for w in want), msc
        got[msc] = []
        for b, (eti_or, trace) in enumerate(want):
            eti = eng.eti(b)
            assert eti.shape == eti_or.shape and np.array_equal(eti, eti_or), "%s form, stream %d (multiplex %d): differs from the oracle" % (msc, b, kinds[b][0])
            ints, ffs = eng.trace(b, len(trace))
            for k, t in enumerate(trace):
                assert tuple(ints[k]) == (t.ok, t.read_frame, t.coarse_timeshift, t.fine_timeshift, t.coarse_freq_shift, t.fifo_count), (msc, b, k)
                assert abs(ffs[k] - t.fine_freq_shift) < 1e-9, (msc, b, k)
            got[msc].append(eti)
        eng.close()
    for msc in MSC_FORMS[1:]:
        for b in range(len(caps)):
            assert np.array_equal(got[msc][b], got[MSC_FORMS[0]][b]), (msc, b)


# ---- (c) FIC forms at the tile edges -------------------------------------------------------------------------------------------
FIC_FRAMES = 513
FIC_KINDS = ["clean", "300 flips", "2500 flips", "random"]


@pytest.fixture(scope="module")
def fic_reference():
    """513 FIC hand-offs (4 blocks each), cycling through clean, correctable, uncorrectable and random blocks, with the oracle's FIBs and CRC
    flags for all of them and the REAL fic_decode's (refh_process on a zero MSC) for 32 of them."""
    O, R = ol.oracle(), ol.ref()
    keep = _keep()
    rng = np.random.default_rng(57)
    cfg = dab.synth_preset(0, seed=58)
    fic = np.zeros((FIC_FRAMES, dab.FIC_BITS), np.uint8)
    for t in range(FIC_FRAMES):
        kind = FIC_KINDS[t % 4]
        if kind == "random":
            fic[t] = rng.integers(0, 2, dab.FIC_BITS, dtype=np.uint8)
            continue
        for q in range(4):
            f = dab.synth_fibs(cfg, 4 * t + q).copy()
            O.or_descramble(ol._ptr(f), 96)
            fic[t, 2304 * q:2304 * (q + 1)] = ol.or_encode(f)[keep]
        if kind != "clean":
            fic[t, rng.integers(0, dab.FIC_BITS, 300 if kind == "300 flips" else 2500)] ^= 1
    fibs = np.zeros((FIC_FRAMES, 12, 32), np.uint8)
    oks = np.zeros((FIC_FRAMES, 12), np.uint8)
    for t in range(FIC_FRAMES):
        O.or_fic_decode(ol._ptr(fic[t]), ol._ptr(fibs[t]), ol._ptr(oks[t]))
    assert oks[0::4].all() and oks[1::4].all() and not oks[2::4].all()
    real = {}
    if R is not None:
        H = R.refh_new()
        zero = np.zeros(dab.MSC_BITS, np.uint8)
        for t in list(range(0, 16)) + list(range(FIC_FRAMES - 16, FIC_FRAMES)):
            idx = R.refh_tfidx(H)
            C.memmove(R.refh_tf_fic(H), ol._ptr(fic[t]), fic[t].size)
            C.memmove(R.refh_tf_msc(H), ol._ptr(zero), zero.size)
            R.refh_process(H)
            real[t] = (np.ctypeslib.as_array(R.refh_fibs(H, idx), (12, 32)).copy(), np.ctypeslib.as_array(R.refh_fib_ok(H, idx), (12,)).copy())
    return fic, fibs, oks, real


@pytest.mark.parametrize("fic_form", ["wave", "lane", "four"])
def test_fic_forms_at_tile_edges_against_the_oracle_and_the_real_fic_decode(fic_form, fic_reference):
    fic, want_fibs, want_ok, real = fic_reference
    eng = dab.Engine(0)
    eng.set_decoder_forms(fic=fic_form)
    for n in (1, 16, 17, 512, 513):          # 4 blocks (one partial tile), 1 full tile, a partial last tile, 128 tiles, 129 tiles
        fibs, ok = eng.stage_fic_decode(fic[:n])
        _assert_report(eng, "wave", fic_form, msc_ran=False)
        for t in range(n):
            assert np.array_equal(fibs[t], want_fibs[t]) and np.array_equal(ok[t], want_ok[t]), (fic_form, n, t, FIC_KINDS[t % 4])
        for t, (rf, rok) in real.items():
            if t < n:
                assert np.array_equal(fibs[t], rf) and np.array_equal(ok[t], rok), (fic_form, n, t, "real fic_decode")
    eng.close()
    if not real:
        pytest.skip("compared with the oracle only: oracle/_ref not built on this box")


# ---- (d) the default rule ------------------------------------------------------------------------------------------------------
# engine.hpp: MSC wave up to 12,288 code words; else four lanes up to 800 groups of 64, two lanes up to 1,536, the lane form above.
# FIC wave up to 3,072 blocks; else four lanes up to 128 tiles of 64 blocks, the lane form above.  The bench multiplex (preset 0: 12
# sub-channels, one code-word plan each, shared by all streams) yields 196 frames per stream in 64 TF, so B streams decode 12 x 196 B code
# words in 12 ceil(196 B / 64) groups, and about 64 B TF = 256 B FIC blocks:
#   B = 1:  2,352 code words            -> wave;  256 blocks             -> wave
#   B = 16: 49 x 12 = 588 groups        -> four;  ~4,096 blocks, 64 tiles -> four
#   B = 32: 98 x 12 = 1,176 groups      -> two;   ~8,192 blocks, 128 tiles -> four
#   B = 64: 196 x 12 = 2,352 groups     -> lane;  ~16,384 blocks, 256 tiles -> lane
@pytest.mark.parametrize("nstreams,msc,fic", [(1, "wave", "wave"), (16, "four", "four"), (32, "two", "four"), (64, "lane", "lane")])
def test_the_default_rule_picks_the_documented_forms(nstreams, msc, fic):
    ntf = 64
    cfgs = [dab.synth_preset(0, seed=9100 + g, cif_count0=(97 * g) % 5000) for g in range(nstreams)]
    nbytes = dab.synth_bytes(cfgs[0], ntf)
    bufs = [dab.DeviceBuffer(nbytes) for _ in range(nstreams)]
    try:
        dab.synth_generate_device(cfgs, ntf, [b.ptr for b in bufs], 0)
        eng = dab.Engine(0)
        eng.set_decoder_forms(msc="auto", fic="auto")
        assert eng.decode_device([b.ptr for b in bufs], [nbytes] * nstreams) == nstreams * 4 * (ntf - 15)
        assert all(cfg.nsub == 12 for cfg in cfgs)
        _assert_report(eng, msc, fic)
        eng.close()
    finally:
        for b in bufs:
            b.free()


# ---- (e) soft decisions ----------------------------------------------------------------------------------------------------------
def test_soft_engine_runs_the_lane_form_when_a_multi_lane_form_is_asked_for():
    iq = dab.synth_generate(dab.synth_preset(1, seed=9301, snr_db=5.0, cif_count0=1234), 24)
    out = {}
    for forms, expect in ((("four", "four"), ("lane", "lane")), (("auto", "auto"), ("wave", "wave"))):
        eng = dab.Engine(0)
        eng.set_soft(True)
        eng.set_decoder_forms(*forms)
        assert eng.decode([iq]) > 0
        _assert_report(eng, *expect)
        out[forms] = eng.eti(0)
        eng.close()
    a, b = out.values()
    assert a.shape == b.shape and a.shape[0] > 0 and np.array_equal(a, b)


def test_a_form_the_decoder_does_not_have_is_refused():
    eng = dab.Engine(0)
    for msc, fic in (("lane", "two"), ("lane", "two-plain"), (5, "lane"), (-2, "lane")):
        with pytest.raises(dab.DabhipError, match="no such form"):
            eng.set_decoder_forms(msc=msc, fic=fic)
    eng.close()
