"""GPU parity tests, second batch: the estimator branches, code profiles and BASELINE configs the first round's tests left
uncovered.  All through the C ABI, compared with the CPU oracle (and, where it exists, with the real reference back end)."""
import ctypes as C
import os

import numpy as np
import pytest

import dabtools_amd as dab
import oracle_lib as ol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    eng = dab.Engine(0)
    yield eng
    eng.close()


def _check_streams(engine, streams, want_all=None):
    """ETI bytes and the full per-call trace of every stream against or_replay."""
    total = engine.decode(streams)
    n = 0
    for b, iq in enumerate(streams):
        want, trace = want_all[b] if want_all else ol.or_replay(iq)
        got = engine.eti(b)
        assert got.shape == want.shape, (b, got.shape, want.shape)
        assert np.array_equal(got, want), "stream %d ETI bytes differ" % b
        ints, ffs = engine.trace(b, max(len(trace), 1))
        for k, t in enumerate(trace):
            assert tuple(ints[k]) == (t.ok, t.read_frame, t.coarse_timeshift, t.fine_timeshift, t.coarse_freq_shift, t.fifo_count), (b, k)
            assert abs(ffs[k] - t.fine_freq_shift) < 1e-9, (b, k)
        n += len(want)
    assert total == n
    return n


def test_coarse_frequency_estimator_and_forced_resync_match_oracle(engine):
    """dab_coarse_freq_sync_2 (sdr_sync.c:205-258) for k != 0 and the branch it drives (input_sdr.c:106-109: |k| > 1 ->
    force_timesync, the next processed frame runs the full coarse time search): captures with a carrier offset, software
    AFC OFF, every call's (ok, coarse_timeshift, fine_timeshift, coarse_freq_shift, fifo_count, fine_freq_shift) == oracle."""
    offsets = (1000.0, -1000.0, 2300.0, -6000.0, 13700.0, 500.0, -14500.0)
    streams, wants = [], []
    for i, cfo in enumerate(offsets):
        iq = dab.synth_generate(dab.synth_preset(1, seed=700 + i, cfo_hz=cfo, snr_db=25.0, skip_samples=(0, 40000)[i & 1]), 22)
        streams.append(iq)
        wants.append(ol.or_replay(iq))
    seen = set()
    forced = 0
    for (_, trace) in wants:
        seen |= {t.coarse_freq_shift for t in trace}
        # a call that found |k| > 1 is followed by a processed frame whose coarse time search was forced
        forced += sum(1 for a, b in zip(trace, trace[1:]) if abs(a.coarse_freq_shift) > 1 and b.coarse_timeshift != 0)
    assert {1, -1, 2, -6, 14} <= seen and forced >= 3          # the oracle really went through those branches
    _check_streams(engine, streams, wants)


def _cut(iq, tf, sample, nsamples):
    p = 2 * (tf * 196608 + sample)
    return np.concatenate([iq[:p], iq[p + 2 * nsamples:]])


def test_resync_while_locked_matches_oracle(engine):
    """Samples vanish (or are inserted) mid-stream AFTER lock: coarse re-synchronisation with a large positive shift, in
    one case larger than what the FIFO still holds after the skip, so the frame buffer keeps skipped bytes
    (sdr_fifo.c:49-55).  ETI bytes and traces == oracle, for the batch engine, a streaming session and the S2/S3 seams."""
    base = dab.synth_generate(dab.synth_preset(1, seed=1), 40)
    rng = np.random.default_rng(3)
    caps = [_cut(base, 21, 30000, 10000),                                       # the advisor's case: shift 373,220 > len 282,128
            _cut(base, 18, 100, 70000), _cut(base, 25, 190000, 3000),
            np.concatenate([base[:2 * 20 * 196608], rng.integers(100, 156, 2 * 50000, dtype=np.uint8), base[2 * 20 * 196608:]]),
            _cut(_cut(base, 17, 5000, 12000), 29, 60000, 130000)]
    wants = [ol.or_replay(c) for c in caps]
    assert all(any(t.coarse_timeshift != 0 for t in tr[12:]) for _, tr in wants)    # a resync after lock in every capture
    assert all(len(w) >= 20 for w, _ in wants)
    _check_streams(engine, caps, wants)
    # streaming session, segments unrelated to the call size
    st = dab.Stream(len(caps))
    got = [[] for _ in caps]
    pos = 0
    for n in (5000000, 262144 * 7, 3333334, 10 ** 9):
        st.feed([c[pos:pos + n] for c in caps])
        for b in range(len(caps)):
            got[b].append(st.eti(b))
        pos += n
    for b in range(len(caps)):
        assert np.array_equal(np.concatenate(got[b]), wants[b][0]), b
    st.close()
    # the seams, like dab2eti.c:60-130
    sdr, d = dab.Sdr(0), dab.Dab(0)
    iq, (want, trace) = caps[0], wants[0]
    for k, off in enumerate(range(0, iq.size - dab.CHUNK_BYTES + 1, dab.CHUNK_BYTES)):
        ok = sdr.demod(iq[off:off + dab.CHUNK_BYTES])
        t = trace[k]
        assert ok == t.ok and sdr.state[:3] == (t.coarse_timeshift, t.fine_timeshift, t.coarse_freq_shift), k
        if ok:
            d.fic[:] = sdr.fic
            d.msc[:] = sdr.msc
            d.process_frame()
    assert np.array_equal(np.array(d.frames), want)
    sdr.close()
    d.close()


def _profile_ensembles():
    """Every UEP table index (0..63), every EEP level with n = 1, 2, 8 (n = 1 at 2-A is the 8 kbit/s special case of
    dab_tables.c:98-100): packed into as few ensembles as 864 CU and 64 SubChIds allow."""
    uep = dab.host_table(0)
    items = [(0, i, int(uep[i][1])) for i in range(64)]
    mult = [12, 8, 6, 4, 27, 21, 18, 15]
    items += [(1, lev, mult[lev] * n) for lev in range(8) for n in (1, 2, 8)]
    ensembles, cur, cu = [], [], 0
    for it in sorted(items, key=lambda x: -x[2]):
        if cu + it[2] > 864 or len(cur) == 18:
            ensembles.append(cur)
            cur, cu = [], 0
        cur.append(it + (cu,))
        cu += it[2]
    ensembles.append(cur)
    return ensembles


def test_all_uep_and_eep_profiles_through_process_frame(forms=None):
    """dab_process_frame (dab.c:35-98 -> create_eti misc.c:218-314 -> uep_/eep_depuncture depuncture.c:84-132) for ALL 64
    UEP profiles and 8 EEP levels x n in {1, 2, 8}: structured FIC, RANDOM MSC bits (so the decoder output is whatever
    the scalar viterbi.c decides, ties included).  HIP back end == the REAL reference objects, frame by frame."""
    R = ol.ref()
    O = ol.oracle()
    dep = np.zeros(3096, np.uint8)
    O.or_fic_depuncture(ol._ptr(dep), ol._ptr(np.zeros(2304, np.uint8)))
    keep = dep != 128
    rng = np.random.default_rng(21)
    ensembles = _profile_ensembles()
    covered = set()
    for ei, ens in enumerate(ensembles):
        cfg = dab.synth_preset(1, seed=900 + ei, cif_count0=240 + ei)      # the CIF counter wraps 249 -> 0 inside the run
        cfg.nsub = len(ens)
        for k, (slform, idx, size, start) in enumerate(ens):
            cfg.sub[k].id = (7 * k + ei) % 64 if len(ens) <= 9 else k * 3
            cfg.sub[k].start_cu = start
            cfg.sub[k].slform = slform
            cfg.sub[k].uep_index = idx if slform == 0 else 0
            cfg.sub[k].eep_protlev = idx if slform == 1 else 0
            cfg.sub[k].size_cu = size
            covered.add((slform, idx, size))
        assert len({cfg.sub[k].id for k in range(cfg.nsub)}) == cfg.nsub
        frames_or = []
        CB = C.CFUNCTYPE(None, C.POINTER(C.c_uint8), C.c_void_p)
        cb = CB(lambda p, u: frames_or.append(np.ctypeslib.as_array(p, (6144,)).copy()))
        od = O.or_dab_new(C.cast(cb, C.c_void_p), None)
        H = R.refh_new() if R is not None else None
        d = dab.Dab(0, forms=forms)
        for t in range(16):
            fic = np.zeros(9216, np.uint8)
            for q in range(4):
                f = dab.synth_fibs(cfg, 4 * t + q).copy()
                O.or_descramble(ol._ptr(f), 96)
                fic[2304 * q:2304 * (q + 1)] = ol.or_encode(f)[keep]
            msc = rng.integers(0, 2, 221184, dtype=np.uint8)
            C.memmove(O.or_dab_tf_fic(od), ol._ptr(fic), fic.size)
            C.memmove(O.or_dab_tf_msc(od), ol._ptr(msc), msc.size)
            O.or_dab_process_frame(od)
            if H is not None:
                C.memmove(R.refh_tf_fic(H), ol._ptr(fic), fic.size)
                C.memmove(R.refh_tf_msc(H), ol._ptr(msc), msc.size)
                R.refh_process(H)
            d.fic[:] = fic
            d.msc[:] = msc
            r = d.process_frame()
            if forms is not None:        # (a caller that pinned the decoder forms: exactly those ran)
                assert d.decoder_forms() == ({forms[0]} if r > 0 else set(), {forms[1]}), (ei, t)
        got = np.array(d.frames)
        assert got.shape == (12, 6144), (ei, got.shape)
        assert np.array_equal(got, np.array(frames_or)), "ensemble %d vs oracle" % ei
        if H is not None:
            n = R.refh_neti(H)
            want = np.ctypeslib.as_array(R.refh_eti(H), (n, 6144))
            assert n == 12 and np.array_equal(got, want), "ensemble %d vs the real reference" % ei
        assert (got[0][5] & 0x7f) == len(ens)
        O.or_dab_free(od)
        d.close()
    assert len(covered) == 64 + 24 and len(ensembles) <= 16
    if R is None:
        pytest.skip("compared with the oracle only: oracle/_ref not built on this box")


def test_config4_full_size_5db_soft_and_hard():
    """BASELINE configs[4] as written: batch = 256 synthetic streams x 64 TF at 5 dB AWGN, soft-decision Viterbi, on one GPU.
    (a) every ETI frame is well formed; (b) frames-out and payload BER within stated bounds; (c) soft >= hard;
    (d) the HARD decode (reference semantics) of 8 of those streams is byte-identical to the CPU oracle."""
    import eti_check
    from dabtools_amd import shard
    nstreams, ntf, ncheck, noracle = 256, 64, 16, 8

    def cfg_of(g, snr):
        return dab.synth_preset(0, seed=shard.stream_seed(4, g), cif_count0=(97 * g) % 5000, snr_db=snr)

    cfgs = [cfg_of(g, 5.0) for g in range(nstreams)]
    bufs = [dab.DeviceBuffer(dab.synth_bytes(c, ntf)) for c in cfgs]      # device memory through the library itself
    dab.synth_generate_device(cfgs, ntf, [b.ptr for b in bufs])
    ptrs, sizes = [b.ptr for b in bufs], [b.nbytes for b in bufs]
    eng = dab.Engine(0)

    def stats(b):
        cfg = cfg_of(b, 1000.0)
        fib_index = {dab.synth_fibs(cfg, c).tobytes(): c for c in range(4 * ntf)}
        frames = good = err = bits = 0
        for e in eng.eti(b):
            p = eti_check.parse(e)                                            # (a) raises on a malformed frame
            frames += 1
            cif = fib_index.get(p["fic"].tobytes())
            if cif is None or p["nst"] != cfg.nsub:
                continue
            wrong = 0
            for k, data in enumerate(p["subch"]):
                want = dab.synth_payload(cfg, cif, k)
                wrong += int(np.unpackbits(np.bitwise_xor(data, want)).sum())
                bits += 8 * want.size
            err += wrong
            good += int(wrong == 0)
        return frames, good, err, bits

    eng.set_soft(True)
    total_soft = eng.decode_device(ptrs, sizes)
    soft = [stats(b) for b in range(ncheck)]
    eng.set_soft(False)
    total_hard = eng.decode_device(ptrs, sizes)
    hard = [stats(b) for b in range(ncheck)]
    expected = 4 * (ntf - 15)
    sf, sb = sum(s[0] for s in soft), sum(s[2] for s in soft) / max(1, sum(s[3] for s in soft))
    hf, hb = sum(h[0] for h in hard), sum(h[2] for h in hard) / max(1, sum(h[3] for h in hard))
    print("config4 5 dB: soft frames %d/%d BER %.2e total %d | hard frames %d BER %.2e total %d" % (sf, ncheck * expected, sb, total_soft, hf, hb, total_hard))
    # (b) stated bounds at 5 dB over the 2.048 MHz band (6.25 dB per carrier): the soft FIC never loses lock, payload BER of
    #     the mixed-protection multiplex stays below 6e-3; hard decisions (the reference's) lose lock and are >= 3x worse
    assert total_soft >= 0.98 * nstreams * expected and sf >= 0.98 * ncheck * expected
    assert sb < 6e-3
    assert total_soft >= total_hard and sf >= hf and sb * 3 < hb                # (c)
    # (d) reference semantics, byte for byte, at the SNR where decisions sit closest to zero
    for b in range(noracle):
        want, trace = ol.or_replay(bufs[b].download())
        got = eng.eti(b)
        assert got.shape == want.shape and np.array_equal(got, want), "stream %d: hard-decision ETI differs from the oracle" % b
    eng.close()


@pytest.mark.parametrize("seam", ["S1", "S3"])
def test_reference_callers_over_the_hip_seams(seam):
    """The drop-in proven literally.  S1: the reference's own, unmodified fic.c / misc.c / dab.c / depuncture.c (compiled where
    they lie by oracle/Makefile) call viterbi() / init_viterbi() of integration/viterbi_hip.c, i.e. libdabhip, at fic.c:186
    and misc.c:262 -- the link-time swap of the reference's Makefile:8-16.  S3: integration/dab_hip.c compiled against the
    reference's dab.h stands in for init_dab_state / dab_process_frame.  Both replay the golden demapped frames
    (tests/golden/backend_e2e.npz: 32 TF at 9 dB with a lock loss) and must emit the ETI bytes the all-CPU reference emitted."""
    so = os.path.join(ol.ORACLE_DIR, "_ref", "libdabref_hip%s.so" % seam)
    if not os.path.exists(so):
        pytest.skip("oracle/_ref/libdabref_hip%s.so not built (needs /root/reference at build time)" % seam)
    L = C.CDLL(so)
    L.refh_new.restype = C.c_void_p
    for f in ("refh_tf_fic", "refh_tf_msc", "refh_eti"):
        getattr(L, f).restype = C.POINTER(C.c_uint8)
    for f in ("refh_tf_fic", "refh_tf_msc", "refh_eti", "refh_process", "refh_neti", "refh_locked"):
        getattr(L, f).argtypes = [C.c_void_p]
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backend_e2e.npz"))
    H = L.refh_new()
    assert H
    locked = []
    for row in g["tf_bits"]:
        bits = np.ascontiguousarray(np.unpackbits(row))
        C.memmove(L.refh_tf_fic(H), ol._ptr(bits[:9216]), 9216)
        C.memmove(L.refh_tf_msc(H), ol._ptr(bits[9216:]), 221184)
        L.refh_process(H)
        locked.append(L.refh_locked(H))
    n = L.refh_neti(H)
    got = np.ctypeslib.as_array(L.refh_eti(H), (n, 6144)).copy() if n else np.zeros((0, 6144), np.uint8)
    assert got.shape == g["eti"].shape and np.array_equal(got, g["eti"])
    assert 0 in locked[12:] and locked[-1] == 1                # the run loses lock and regains it


@pytest.mark.parametrize("level", [1, 2])
def test_parity_guard_makes_fp32_decisions_exact(engine, level):
    """The stated float tolerance of the OFDM stage, and its removal, at both guard levels (1 = measured band, 2 = proven band: dabhip.h).  K2 + K2b in
    fp32 against fp64 transforms of the same samples (dabhip_stage_decision_audit) at 5 dB, where decisions sit closest to zero: (a) guard off: the raw
    fp32 decisions may disagree, but only on carriers the guard rule flags, and every fp32 error stays a factor >= 2 inside the MEASURED level's
    constants (a fortiori inside the proven ones, which are >= the rigorous bound of tools/fft_error_bound.py); (b) guard on: zero disagreements.
    tools/decision_audit.py runs the same on > 10^10 decisions at both levels."""
    engine.set_parity_guard(level)
    c_bin, c_prod = dab.guard_constants(level)
    assert (c_bin, c_prod) == (pytest.approx(5.0e-6), pytest.approx(5.0e-7)) if level == 1 else (c_bin >= 6.5072e-5 and c_prod >= 1.1921e-7)
    ntf = 24
    caps = [dab.synth_generate(dab.synth_preset(0, seed=1200 + i, snr_db=snr, amplitude=amp), ntf) for i, (snr, amp) in enumerate(((5.0, 1.0), (5.0, 0.3), (7.0, 1.0), (1000.0, 1.0)))]
    frames = np.concatenate(caps)
    off = engine.decision_audit(frames=frames, guard=False)
    on = engine.decision_audit(frames=frames, guard=True)
    print("audit guard off:", off, "guard on:", on)
    assert off["decisions"] == 4 * ntf * 230400 == on["decisions"]
    assert off["disagree_outside_guard"] == 0                                 # (a) nothing slips past the rule
    assert off["max_bin_err"] < 2.5e-6 and off["max_dec_err"] < 2.5e-6          # kGuardC = 5e-6
    assert off["max_prod_err"] < 2.5e-7                                       # kGuardProd = 5e-7
    assert 0 < off["flagged_by_rule"] < 1e-3 * off["decisions"]
    assert on["disagree"] == 0 and on["listed"] == off["flagged_by_rule"]     # (b)
    engine.set_parity_guard(True)


def test_parity_guard_end_to_end_and_off_switch():
    """Guard on (both levels) vs off on noisy captures: same frames out; the guard re-decides a small, non-zero number of decisions -- the proven level
    roughly 13 x as many as the measured one; with it on, fused and two-kernel OFDM stages and the oracle agree byte for byte."""
    caps = [dab.synth_generate(dab.synth_preset(1, seed=1300 + i, snr_db=snr), 30) for i, snr in enumerate((5.0, 6.0, 9.0))]
    replays = [ol.or_replay(c) for c in caps]
    wants = [r[0] for r in replays]
    demodulated = sum(t.ok for _, trace in replays for t in trace)            # sdr_demod calls that returned 1: one TF of decisions each
    eng = dab.Engine(0)
    assert eng.parity_guard_level() == dab.guard_default_level() in (1, 2)
    counts = {}
    for level in (1, 2):
        eng.set_parity_guard(level)
        assert eng.parity_guard_level() == level
        for fused in (True, False):
            eng.set_fused(fused)
            eng.decode(caps)
            flagged, decisions = eng.guard_stats()
            assert 0 < flagged < 2e-3 * decisions, (level, fused, flagged, decisions)
            assert decisions == demodulated * 230400, (fused, decisions, demodulated)
            assert eng.guard_overflows() == 0
            counts[level, fused] = flagged
            for b, w in enumerate(wants):
                assert np.array_equal(eng.eti(b), w), (level, fused, b)
    assert 6 * counts[1, True] < counts[2, True] < 30 * counts[1, True], counts       # the band is 13.2 x as wide
    eng.set_parity_guard(False)
    eng.decode(caps)
    assert eng.guard_stats()[0] == 0
    assert [eng.eti_count(b) for b in range(3)] == [len(w) for w in wants]     # fp32 flips are far too rare to move the lock
    eng.close()


def test_soft_decisions_one_kernel_and_two_kernel_stages_agree():
    """Soft decisions: the one-kernel OFDM stage (k_fused.hip, DABHIP_FUSED_SOFT build) and K2 + K2b produce the same 4-bit values
    (the scale comes from the symbols' sample energies, added up as integers in every kernel), hence the same ETI bytes -- on
    noisy captures where the quantised values matter; and a streaming session gives the one-shot result."""
    caps = [dab.synth_generate(dab.synth_preset(p, seed=1400 + i, snr_db=snr, skip_samples=sk), 34)
            for i, (p, snr, sk) in enumerate(((1, 5.5, 0), (0, 6.5, 41000), (1, 8.0, 0), (1, 1000.0, 123)))]
    eng = dab.Engine(0)
    eng.set_soft(True)
    eng.set_fused(False)
    eng.decode(caps)
    want = [eng.eti(b) for b in range(len(caps))]
    assert eng.stage_ms()["demap"] > 0.02
    eng.set_fused(True)
    eng.decode(caps)
    for b, w in enumerate(want):
        assert len(w) > 40 and np.array_equal(eng.eti(b), w), b
    st = dab.Stream(len(caps), soft=True)
    got, pos = [[] for _ in caps], 0
    for n in (4000000, 262144 * 9, 10 ** 9):
        st.feed([c[pos:pos + n] for c in caps])
        for b in range(len(caps)):
            got[b].append(st.eti(b))
        pos += n
    for b, w in enumerate(want):
        assert np.array_equal(np.concatenate(got[b]), w), b
    st.close()
    eng.close()


@pytest.mark.gpu
def test_device_buffers_and_stream_ceiling():
    """The small C-ABI helpers bench.py and the tests lean on: device memory through the library, and the streaming-rate probe
    whose figures the K2 roofline is read against (sane = between 0.1 and 9 TB/s)."""
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
    buf = dab.DeviceBuffer(data.size)
    buf.upload(data)
    assert np.array_equal(buf.download(), data)
    buf.free()
    r = dab.stream_ceiling(0, 256 << 20, 3)
    assert set(r) == {"fill", "copy", "k2_mix"}
    assert all(100.0 < v < 9000.0 for v in r.values()), r      # a plausibility check only: the first kernels of a fresh process run slow
