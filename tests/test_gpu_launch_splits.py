"""Every loop that splits a decode into several launches, and the copy-engine form of the scan's download, run on test-sized input.

A decode larger than one launch can hold is cut into pieces (launch_limits.hpp): the MSC decoder into slices of survivor-record rows, the regroup
and the FIC group into pieces of tiles, a session's device gather into pieces of descriptors, the two-kernel OFDM stage into chunks of TFs (its FIC
pre-pass into chunks 19 x as long), and scan results of more than 2^18 words come back by copy-engine commands.  At the default limits every one of
these loops runs once on anything a test can afford, so its offsets are only ever computed for piece 0.  Here the limits are lowered per engine
(Engine.set_launch_limits) and the output is compared byte for byte with the oracle's replay of the same captures and with the same engine at the
default limits -- and every test reads from Engine.launch_report() that the split it is about really happened, and in how many pieces.

  (a) decoder slices: about two groups per slice, exactly one longest group's rows, one row -- every hard form, soft lane; the wave form stays one slice
  (b) regroup and FIC-group pieces of 8 tiles over 8, 9, 16 and 19 tiles, partial tiles, hard and soft; the FIC decoder's lane and four-lane forms
  (c) two-kernel OFDM stage in chunks of 5 TF over 5, 6, 10, 11 and 96 TF, guard levels 1 and 2, guard off, soft; the stage entries under the same limit
  (d) scan results through the copy engine: split scan, with look-ahead, AFC (not split), rescan after a violation; and once past the real 2^18 words
  (e) device gather in pieces of 3 descriptors in a session fed from device memory at odd alignments
  (f) limits no launch could be made with are refused and leave the engine as it was

No tolerance anywhere: a split must not change a byte."""
import numpy as np
import pytest

import dabtools_amd as dab
import oracle_lib as ol
import test_gpu_decoder_forms as forms
import test_gpu_hostfed as hostfed

pytestmark = pytest.mark.gpu


def _pieces(n, limit):
    return (n + limit - 1) // limit


def _report(obj, what, **expect):
    """The launch report of the last decode, printed, with the counts this test is about asserted."""
    r = obj.launch_report()
    print("launches %-58s %s" % (what, " ".join("%s=%d" % (k, r[k]) for k in dab.LAUNCH_REPORT)))
    for k, v in expect.items():
        assert r[k] == v, (what, k, r[k], v, r)
    return r


def _assert_trace(eng, b, trace, what, tol=1e-9):
    ints, ffs = eng.trace(b, len(trace))
    assert len(ints) == len(trace), (what, b)
    for k, t in enumerate(trace):
        assert tuple(ints[k]) == (t.ok, t.read_frame, t.coarse_timeshift, t.fine_timeshift, t.coarse_freq_shift, t.fifo_count), (what, b, k)
        assert abs(ffs[k] - t.fine_freq_shift) < tol, (what, b, k)


def _assert_eti(eng, wants, what):
    for b, w in enumerate(wants):
        got = eng.eti(b)
        assert got.shape == w.shape and np.array_equal(got, w), "%s: stream %d differs" % (what, b)


# ---- (a) decoder slices ----------------------------------------------------------------------------------------------------------
def _slice_count(steps, max_rows):
    """worklist.hpp's rule restated: groups in launch order, a new slice where the next group's rows would pass max_rows (a slice holds at least one group)."""
    count, rows = 1, 0
    for g, s in enumerate(steps):
        dr = (int(s) + 7) // 8 * 8
        if rows > 0 and rows + dr > max_rows:
            count += 1
            rows = 0
        rows += dr
    return count


@pytest.fixture(scope="module")
def mixed_batch():
    """Four streams x 24 TF at 9 .. 12 dB: two of the dense 20-sub-channel UEP / EEP multiplex (they share its plans: groups of 64 + 8 code words), one of
    each preset; the oracle's hard and soft replays, once."""
    cfgs = [forms._dense_cfg(8801, 9.0), forms._dense_cfg(8802, 12.0), dab.synth_preset(0, seed=8803, snr_db=10.0, cif_count0=1200, skip_samples=31000),
            dab.synth_preset(1, seed=8804, snr_db=11.0, cif_count0=77)]
    caps = [dab.synth_generate(c, 24) for c in cfgs]
    hard = [ol.or_replay(iq) for iq in caps]
    soft = [ol.or_replay_soft(iq)[0] for iq in caps]
    assert all(len(w[0]) >= 24 for w in hard) and all(len(w) >= 24 for w in soft)
    return caps, hard, soft


@pytest.mark.parametrize("msc,soft", [("lane", False), ("two", False), ("two-plain", False), ("four", False), ("lane", True)])
def test_decoder_slices_equal_one_launch_and_the_oracle(msc, soft, mixed_batch):
    caps, hard, soft_want = mixed_batch
    wants = soft_want if soft else [w[0] for w in hard]
    what = "%s%s" % (msc, " soft" if soft else "")
    eng = dab.Engine(0)
    eng.set_soft(soft)
    eng.set_decoder_forms(msc=msc, fic="lane")
    assert eng.decode(caps) == sum(len(w) for w in wants)
    _report(eng, "(a) %s, default rows" % what, decoder=1)
    _assert_eti(eng, wants, what + ", default limit: oracle")
    unsplit = [eng.eti(b) for b in range(len(caps))]
    steps, _ = eng.msc_plan()
    rows = [(int(s) + 7) // 8 * 8 for s in steps]
    # long and short code words (several length classes, the shortest under a tenth of the longest), more than one group per plan, longest first
    assert len(steps) >= 40 and len(set(steps.tolist())) >= 5 and 10 * steps[-1] < steps[0] and list(steps) == sorted(steps, reverse=True)
    longest = rows[0]
    for name, limit in (("two longest groups", 2 * longest), ("one longest group", longest), ("one row", 1)):
        expect = _slice_count(steps, limit)
        if limit == 1:
            assert expect == len(steps)
        elif limit == longest:
            assert rows[1] == longest and expect < len(steps)       # two groups of the longest class: the second does NOT fit beside the first, short ones share
        else:
            assert 4 <= expect < len(steps) // 2
        eng.set_launch_limits(decision_rows=limit)
        assert eng.decode(caps) == sum(len(w) for w in wants)
        _report(eng, "(a) %s, %s (%d rows)" % (what, name, limit), decoder=expect, decoder_planned=expect)      # launches made == the host plan's slices == the rule
        m, _ = eng.decoder_forms(masks=True)
        assert m == 1 << dab.FORMS["lane" if soft else msc]
        _assert_eti(eng, wants, "%s, %s: oracle" % (what, name))
        _assert_eti(eng, unsplit, "%s, %s: default limit" % (what, name))
    if not soft:
        for b, (_, trace) in enumerate(hard):
            _assert_trace(eng, b, trace, what)
    eng.close()


def test_the_wave_form_is_one_slice_whatever_the_row_limit(mixed_batch):
    caps, hard, _ = mixed_batch
    eng = dab.Engine(0)
    eng.set_decoder_forms(msc="wave", fic="wave")
    eng.set_launch_limits(decision_rows=1)
    assert eng.decode(caps) == sum(len(w[0]) for w in hard)
    _report(eng, "(a) wave form, one row", decoder=1)
    _assert_eti(eng, [w[0] for w in hard], "wave form")
    eng.close()


# ---- (b) regroup and FIC-group pieces ----------------------------------------------------------------------------------------------
TILE_LIMIT = 8


@pytest.fixture(scope="module")
def tile_pool():
    """19 captures whose ETI jobs fill a known number of regroup tiles: streams 0 and 1 carry the same multiplex (24 TF: 36 frames each, 72 records = a
    full tile and one of 8), every other stream a multiplex of its own (20 TF: 20 frames = one tile of 20 records, the rest of its job ids -1).  The
    first n streams make n tiles for n >= 2."""
    caps = []
    for i in range(19):
        cfg = dab.synth_preset(1, seed=8900 + i, snr_db=(1000.0, 10.0)[i % 2], cif_count0=(131 * i) % 5000)
        if i >= 2:
            cfg.sub[3].start_cu = 300 + i            # a layout of its own: the job lists of two multiplexes never share a tile
        caps.append(dab.synth_generate(cfg, 24 if i < 2 else 20))
    hard = [ol.or_replay(iq) for iq in caps]
    soft = [ol.or_replay_soft(iq)[0] for iq in caps]
    assert [len(w[0]) for w in hard] == [36, 36] + [20] * 17 and [len(w) for w in soft] == [36, 36] + [20] * 17
    return caps, hard, soft


@pytest.mark.parametrize("soft", [False, True])
def test_regroup_and_fic_group_pieces_in_a_decode(soft, tile_pool):
    caps, hard, soft_want = tile_pool
    low, default = dab.Engine(0), dab.Engine(0)
    for eng in (low, default):
        eng.set_soft(soft)
        eng.set_decoder_forms(msc="lane", fic="lane")
    low.set_launch_limits(regroup_tiles=TILE_LIMIT, fic_group_tiles=TILE_LIMIT)
    for tiles in (8, 9, 16, 2 * 8 + 3):              # one full launch; a second of one tile; two full ones; a partial last one
        sub = caps[:tiles]
        wants = (soft_want if soft else [w[0] for w in hard])[:tiles]
        fic_tiles = _pieces(4 * sum(t.ok for _, trace in hard[:tiles] for t in trace), 64)      # 4 FIC blocks per demodulated TF, tiles of 64 blocks
        what = "%d tiles%s" % (tiles, ", soft" if soft else "")
        assert default.decode(sub) == sum(len(w) for w in wants)
        _report(default, "(b) %s, default" % what, regroup=1, fic_group=1)
        assert default.msc_plan()[1] == tiles
        assert low.decode(sub) == sum(len(w) for w in wants)
        _report(low, "(b) %s, 8 per launch" % what, regroup=_pieces(tiles, TILE_LIMIT), fic_group=_pieces(fic_tiles, TILE_LIMIT))
        assert low.msc_plan()[1] == tiles and fic_tiles > TILE_LIMIT
        _assert_eti(low, wants, what + ": oracle")
        _assert_eti(low, [default.eti(b) for b in range(tiles)], what + ": default limit")
    low.close()
    default.close()


@pytest.fixture(scope="module")
def fic_blocks():
    """300 FIC hand-offs (4 blocks each) -- clean, correctable, uncorrectable, random in turn -- with the oracle's FIBs and CRC flags."""
    O = ol.oracle()
    keep = forms._keep()
    rng = np.random.default_rng(8950)
    cfg = dab.synth_preset(0, seed=8951)
    n = 300
    fic = np.zeros((n, dab.FIC_BITS), np.uint8)
    for t in range(n):
        kind = forms.FIC_KINDS[t % 4]
        if kind == "random":
            fic[t] = rng.integers(0, 2, dab.FIC_BITS, dtype=np.uint8)
            continue
        for q in range(4):
            f = dab.synth_fibs(cfg, 4 * t + q).copy()
            O.or_descramble(ol._ptr(f), 96)
            fic[t, 2304 * q:2304 * (q + 1)] = ol.or_encode(f)[keep]
        if kind != "clean":
            fic[t, rng.integers(0, dab.FIC_BITS, 300 if kind == "300 flips" else 2500)] ^= 1
    fibs = np.zeros((n, 12, 32), np.uint8)
    oks = np.zeros((n, 12), np.uint8)
    for t in range(n):
        O.or_fic_decode(ol._ptr(fic[t]), ol._ptr(fibs[t]), ol._ptr(oks[t]))
    assert oks[0::4].all() and not oks[2::4].all()
    return fic, fibs, oks


@pytest.mark.parametrize("fic_form", ["lane", "four"])
def test_fic_group_pieces_at_their_edges(fic_form, fic_blocks):
    fic, want_fibs, want_ok = fic_blocks
    low, default = dab.Engine(0), dab.Engine(0)
    low.set_launch_limits(fic_group_tiles=TILE_LIMIT)
    # frames -> blocks -> tiles: 128 -> 512 -> 8 (one launch); 129 -> 516 -> 9 (the second piece: 4 blocks); 144 -> 576 -> 9 (the second piece: exactly 64);
    # 256 -> 1024 -> 16 (two full launches); 300 -> 1200 -> 19 (the last piece: 176 blocks, its last tile 48)
    for n, tiles in ((128, 8), (129, 9), (144, 9), (256, 16), (300, 19)):
        assert _pieces(4 * n, 64) == tiles
        out = {}
        for eng, name in ((default, "default"), (low, "8 per launch")):
            eng.set_decoder_forms(fic=fic_form)
            out[name] = eng.stage_fic_decode(fic[:n])
            _report(eng, "(b) FIC %s form, %d blocks, %s" % (fic_form, 4 * n, name), fic_group=1 if eng is default else _pieces(tiles, TILE_LIMIT), regroup=0, decoder=0)
            assert eng.decoder_forms(masks=True)[1] == 1 << dab.FORMS[fic_form]
        fibs, ok = out["8 per launch"]
        for t in range(n):
            assert np.array_equal(fibs[t], want_fibs[t]) and np.array_equal(ok[t], want_ok[t]), (fic_form, n, t, forms.FIC_KINDS[t % 4])
        assert np.array_equal(fibs, out["default"][0]) and np.array_equal(ok, out["default"][1]), (fic_form, n)
    low.close()
    default.close()


# ---- (c) two-kernel OFDM stage in chunks ---------------------------------------------------------------------------------------------
CHUNK = 5


@pytest.fixture(scope="module")
def chunk_cases():
    """Captures that demodulate exactly 5, 6, 10, 11 and 96 TFs (the chunk, one more, a multiple, one more than that, and more than 19 chunks: the FIC
    pre-pass takes 95 + 1), noisy enough (5 .. 6 dB) for the guard to list decisions in every chunk.  {TFs: (captures, hard replays, soft ETI)}"""
    recipes = {5: [(1, 5.5, 0, 7)], 6: [(1, 6.0, 0, 8)], 10: [(1, 5.0, 0, 12)], 11: [(0, 5.5, 0, 13)],
               96: [(1, 5.5, 0, 26), (0, 6.0, 41000, 28), (1, 9.0, 0, 26), (1, 5.0, 0, 26)]}
    cases = {}
    for total, streams in recipes.items():
        caps = [dab.synth_generate(dab.synth_preset(p, seed=9000 + total + i, snr_db=snr, skip_samples=sk, cif_count0=50 * i), ntf) for i, (p, snr, sk, ntf) in enumerate(streams)]
        hard = [ol.or_replay(iq) for iq in caps]
        assert sum(t.ok for _, trace in hard for t in trace) == total, (total, [sum(t.ok for t in trace) for _, trace in hard])
        cases[total] = (caps, hard, [ol.or_replay_soft(iq)[0] for iq in caps])
    assert sum(len(w[0]) for w in cases[96][1]) >= 64
    return cases


def _sample_tfs(ntf):
    """TFs whose demapped values are compared: all of a short stream, else the ones at both sides of the chunk borders near its ends and its middle."""
    if ntf <= 12:
        return list(range(ntf))
    return sorted({0, 1, CHUNK - 1, CHUNK, 2 * CHUNK, ntf // 2, ntf - CHUNK - 1, ntf - 2, ntf - 1})


@pytest.mark.parametrize("mode", ["guard1", "guard2", "guard0", "soft"])
def test_two_kernel_ofdm_chunks_equal_one_launch_and_the_oracle(mode, chunk_cases):
    low, default = dab.Engine(0), dab.Engine(0)
    for eng in (low, default):
        eng.set_fused(False)
        eng.set_demod_all(True)                      # every TF through the MSC launches: the chunk count is that of the TFs, not of the lockable ones
        eng.set_soft(mode == "soft")
        if mode != "soft":
            eng.set_parity_guard(int(mode[-1]))
    low.set_launch_limits(fft_chunk_tfs=CHUNK)
    for total, (caps, hard, soft_want) in chunk_cases.items():
        wants = soft_want if mode == "soft" else [w[0] for w in hard]
        what = "%s, %d TF" % (mode, total)
        assert default.decode(caps) == sum(len(w) for w in wants)
        _report(default, "(c) %s, default chunk" % what, ofdm_chunks=1, fic_prepass=1)
        assert low.decode(caps) == sum(len(w) for w in wants)
        _report(low, "(c) %s, chunks of 5" % what, ofdm_chunks=_pieces(total, CHUNK), fic_prepass=_pieces(total, 19 * CHUNK))
        for eng in (low, default):
            flagged, decisions = eng.guard_stats()
            if mode in ("guard1", "guard2"):
                assert flagged > 0 and eng.guard_overflows() == 0 and decisions == total * 230400, (what, flagged, decisions)
            else:
                assert flagged == 0, what
        if mode in ("guard1", "guard2"):
            assert low.guard_stats() == default.guard_stats(), what
        if mode != "guard0":                         # (raw fp32 decisions claim no reference semantics: compared with the unsplit run only)
            _assert_eti(low, wants, what + ": oracle")
        _assert_eti(low, [default.eti(b) for b in range(len(caps))], what + ": default chunk")
        for b, (_, trace) in enumerate(hard):
            for t in _sample_tfs(sum(x.ok for x in trace)):
                a, z = low.demapped_tf(b, t), default.demapped_tf(b, t)
                assert np.array_equal(a[0], z[0]) and np.array_equal(a[1], z[1]), (what, b, t)
    low.close()
    default.close()


def test_chunks_of_the_lockable_frames_and_their_completion_on_demand(chunk_cases):
    """With the lock-in skip on, the MSC launches cover the lockable frames only (the first 9 TFs of each of the four streams are deferred): chunks of 5 over
    those 60, and the deferred 36 completed in chunks of 5 when demapped_tf asks for one."""
    caps, hard, _ = chunk_cases[96]
    low, default = dab.Engine(0), dab.Engine(0)
    for eng in (low, default):
        eng.set_fused(False)
    low.set_launch_limits(fft_chunk_tfs=CHUNK)
    for eng in (low, default):
        assert eng.decode(caps) == sum(len(w[0]) for w in hard) and eng.msc_deferred() == 36
    _report(low, "(c) lock-in skip, 60 of 96 TF in chunks of 5", ofdm_chunks=12, fic_prepass=2)
    _assert_eti(low, [w[0] for w in hard], "lock-in skip: oracle")
    for b in range(len(caps)):
        for t in (8, 0, 4):                          # deferred TFs: the first request completes all 36
            a, z = low.demapped_tf(b, t), default.demapped_tf(b, t)
            assert np.array_equal(a[0], z[0]) and np.array_equal(a[1], z[1]), (b, t)
    _report(low, "(c) ... and the deferred 36 on demand", ofdm_chunks=12 + _pieces(36, CHUNK))
    low.close()
    default.close()


def test_stage_entries_under_the_chunk_limit(chunk_cases):
    """stage_ofdm_fft + stage_demap, the decision audit and fft_roofline with the chunk limit lowered: the audit and the roofline run in chunks of 5 (and
    say so), the spectra entry is one launch as ever; every result equals the default engine's."""
    frames = dab.synth_generate(dab.synth_preset(1, seed=9050, snr_db=5.5), 11)
    low, default = dab.Engine(0), dab.Engine(0)
    low.set_launch_limits(fft_chunk_tfs=CHUNK)
    out = {}
    for eng in (low, default):
        spectra, _ = eng.stage_ofdm_fft(frames)
        fic, msc = eng.stage_demap(spectra)
        audits = []
        for guard in (False, True):
            audits.append(eng.decision_audit(frames, guard=guard))
            _report(eng, "(c) decision audit of 11 TF, guard %d, %s" % (guard, "chunks of 5" if eng is low else "default"), ofdm_chunks=3 if eng is low else 1)
        out[eng is low] = (spectra, fic, msc, audits)
    assert np.array_equal(out[True][0], out[False][0]) and np.array_equal(out[True][1], out[False][1]) and np.array_equal(out[True][2], out[False][2])
    assert out[True][3] == out[False][3], (out[True][3], out[False][3])
    off, on = out[True][3]
    assert off["decisions"] == on["decisions"] == 11 * 230400 and on["disagree"] == 0 and on["listed"] == off["flagged_by_rule"] > 0
    caps, hard, _ = chunk_cases[11]
    for eng in (low, default):
        eng.decode(caps)
        before = eng.launch_report()
        launches, tfs, _ = eng.fft_roofline(reps=2)
        assert (launches, tfs) == ((2 * 3, 2 * 11) if eng is low else (2, 2 * 11))
        assert eng.launch_report() == before, "fft_roofline leaves the decode's launch report alone"
    low.close()
    default.close()


# ---- (d) scan results through the copy engine ----------------------------------------------------------------------------------------
def _scan_case(shape):
    """(captures, K1's chain mode, AFC) of one shape of scan_fetch's argument list"""
    if shape == "rescan":      # off-tune captures of test_sync_verification_fp32_first_pass_and_its_fp64_fallback: the chain's assumption breaks, those streams are scanned again
        return [dab.synth_generate(dab.synth_preset(1, seed=1900 + i, cfo_hz=cfo, snr_db=snr, skip_samples=sk), 22)
                for i, (cfo, snr, sk) in ((1, (2300.0, 25.0, 40000)), (2, (-6000.0, 20.0, 0)), (5, (150.0, 1000.0, 99)), (7, (0.0, 1000.0, 0)))], 0, False
    if shape == "afc":
        return [dab.synth_generate(dab.synth_preset(1, seed=450 + i, cif_count0=77 * i, cfo_hz=cfo, snr_db=snr, skip_samples=skip), 30)
                for i, (cfo, snr, skip) in enumerate(((3400.0, 25.0, 0), (-260.0, 15.0, 30000)))], -1, True
    plain = [dab.synth_generate(dab.synth_preset(p, seed=9100 + p, snr_db=snr, skip_samples=sk, cif_count0=400), 22) for p, snr, sk in ((1, 15.0, 0), (0, 1000.0, 70001))]
    return plain, (1 if shape == "split + look-ahead" else 0), False


@pytest.mark.parametrize("shape", ["split", "split + look-ahead", "afc", "rescan"])
def test_scan_results_through_the_copy_engine(shape):
    caps, spec, afc = _scan_case(shape)
    knobs = dict(spec=spec, afc=afc)
    replays = [ol.or_replay_afc(iq) if afc else ol.or_replay(iq) for iq in caps]
    calls = {}
    for form, words in ((dab.FETCH_KERNEL, 0), (dab.FETCH_COPY_ENGINE, 1)):
        eng = dab.Engine(0)
        eng.set_afc(knobs["afc"])
        eng.set_sync_speculation(knobs["spec"])
        eng.set_launch_limits(fetch_words=words)
        assert eng.decode(caps) == sum(len(r[0]) for r in replays)
        st = eng.stage_ms()
        calls[form] = (st["sync_fp64_calls"], st["sync_spec_calls"])
        r = _report(eng, "(d) %s, fetch limit %d" % (shape, words), fetch_form=form, fetches=2 if shape == "rescan" else 1)
        for b, rep in enumerate(replays):
            _assert_trace(eng, b, rep[1], shape, 1e-6 if knobs["afc"] else 1e-9)
            if knobs["afc"]:
                assert np.array_equal(eng.trace_nco(b, len(rep[1])), rep[2]), (shape, b)
        _assert_eti(eng, [rep[0] for rep in replays], "%s, fetch form %d" % (shape, r["fetch_form"]))
        eng.close()
    assert calls[dab.FETCH_KERNEL] == calls[dab.FETCH_COPY_ENGINE], calls          # both travel in the fetched words
    if shape == "split + look-ahead":
        assert calls[dab.FETCH_COPY_ENGINE][1] > 0
    if shape == "afc":
        assert calls[dab.FETCH_COPY_ENGINE] == (0, 0)


def test_scan_results_past_the_real_threshold():
    """No knob: enough streams that the scan's results pass 2^18 words.  All but three stream pointers alias ONE device buffer of mid-scale silence (60 calls
    that never find a null symbol: K1 time only); three are real captures."""
    ncalls = 60
    state_words = dab.host_stream_state_bytes() // 4
    nstreams = (1 << 18) // (2 * ncalls + 1 + state_words) + 2
    assert nstreams * ncalls * 2 + nstreams + 1 + nstreams * state_words > 1 << 18 and 1000 < nstreams < 4000
    silence = np.full(ncalls * 262144, 128, np.uint8)
    silent_eti, silent_trace = ol.or_replay(silence)
    assert len(silent_eti) == 0 and len(silent_trace) == ncalls and not any(t.ok for t in silent_trace)
    real = [dab.synth_generate(dab.synth_preset(p, seed=9200 + p + sk, snr_db=snr, skip_samples=sk), 24) for p, snr, sk in ((1, 10.0, 0), (0, 1000.0, 5000), (1, 7.0, 90001))]
    replays = [ol.or_replay(iq) for iq in real]
    where = {0: 0, nstreams // 2: 1, nstreams - 2: 2}        # the real captures' places in the batch
    bufs = [dab.DeviceBuffer(silence.size)] + [dab.DeviceBuffer(iq.size) for iq in real]
    try:
        bufs[0].upload(silence)
        for buf, iq in zip(bufs[1:], real):
            buf.upload(iq)
        ptrs = [bufs[1 + where[b]].ptr if b in where else bufs[0].ptr for b in range(nstreams)]
        sizes = [real[where[b]].size if b in where else silence.size for b in range(nstreams)]
        eng = dab.Engine(0)
        assert eng.decode_device(ptrs, sizes) == sum(len(r[0]) for r in replays)
        _report(eng, "(d) %d streams x %d calls, default limits" % (nstreams, ncalls), fetch_form=dab.FETCH_COPY_ENGINE)
        for b, k in where.items():
            _assert_trace(eng, b, replays[k][1], "real capture %d" % k)
            assert np.array_equal(eng.eti(b), replays[k][0]), k
        rng = np.random.default_rng(9210)
        aliased = [b for b in range(nstreams) if b not in where]
        for b in [aliased[0], aliased[-1]] + [aliased[i] for i in rng.choice(len(aliased), 20, replace=False)]:
            _assert_trace(eng, b, silent_trace, "silence")
            assert eng.eti_count(b) == 0, b
        eng.close()
    finally:
        for buf in bufs:
            buf.free()


# ---- (e) device gather in pieces -------------------------------------------------------------------------------------------------------
GATHER_LIMIT = 3


def test_device_gather_pieces_in_a_session():
    """The cut points and shifts of test_stream_session_with_prefetched_segments_equals_one_shot_decode's device-fed part, the gathers in pieces of 3
    descriptors.  A feed makes two gathers: the segments (one descriptor per stream that has bytes) and the history moved in front of them (one per stream
    the front end may still read earlier bytes of).  Six streams: 6 descriptors = exactly two launches; one more cut at 7,850,000 bytes, past the end of
    every stream but one, gives a gather of 1."""
    caps = hostfed._caps()[:6]
    assert sorted(c.size > 7850000 for c in caps) == [False] * 5 + [True]
    oracle = {b: ol.or_replay(caps[b])[0] for b in (0, 2, 5)}
    eng = dab.Engine(0)
    eng.decode(caps)
    want = [eng.eti(b) for b in range(len(caps))]
    eng.close()
    for b, w in oracle.items():
        assert np.array_equal(want[b], w), b
    cuts = [0, 3000000, 3000000 + 262144 * 5, 5500000, 5500001, 6900000, 7850000, 10 ** 9]
    got = {}
    for limit in (0, GATHER_LIMIT):
        st = dab.Stream(len(caps))
        st.set_launch_limits(gather_descs=limit)
        got[limit] = [[] for _ in caps]
        keep, seen = [], set()
        fed = [0] * len(caps)
        for k, (a, z) in enumerate(zip(cuts, cuts[1:])):
            parts = [c[a:z] for c in caps]
            bufs = [dab.DeviceBuffer(max(p.size, 16) + 32) for p in parts]
            shift = [(3 * b + 5 * k + 1) % 17 for b in range(len(bufs))]
            for buf, p, sh in zip(bufs, parts, shift):
                if p.size:
                    tmp = np.zeros(p.size + 32, np.uint8)
                    tmp[sh:sh + p.size] = p
                    buf.upload(tmp)
            keep.append(bufs)
            nseg = sum(1 for p in parts if p.size)
            nhist = sum(1 for b in range(len(caps)) if k > 0 and fed[b] - st.need_from(b) > 0)      # streams whose earlier bytes K1 may still read
            st.feed_ptrs([b.ptr + sh for b, sh in zip(bufs, shift)], [p.size for p in parts], on_device=True)
            fed = [n + p.size for n, p in zip(fed, parts)]
            per = limit or 65535
            _report(st, "(e) feed %d: %d segments + %d history moves, %d per launch" % (k, nseg, nhist, per),
                    gather=_pieces(nseg, per) + _pieces(nhist, per), gather_calls=(nseg > 0) + (nhist > 0))
            seen.update((nseg, nhist))
            for b in range(len(caps)):
                got[limit][b].append(st.eti(b))
        st.close()
        for bufs in keep:
            for buf in bufs:
                buf.free()
        assert {1, 6} <= seen, seen                  # a multiple of 3 and a single descriptor
    for b, w in enumerate(want):
        assert np.array_equal(np.concatenate(got[GATHER_LIMIT][b]), w), b
        assert np.array_equal(np.concatenate(got[0][b]), w), b


# ---- (f) refusals ----------------------------------------------------------------------------------------------------------------------
def test_limits_no_launch_could_be_made_with_are_refused():
    iq = dab.synth_generate(dab.synth_preset(1, seed=9300, snr_db=9.0), 20)
    want, _ = ol.or_replay(iq)
    eng = dab.Engine(0)
    eng.set_launch_limits(regroup_tiles=8, gather_descs=3)
    for bad in (dict(regroup_tiles=12), dict(regroup_tiles=4), dict(regroup_tiles=-8), dict(regroup_tiles=32776), dict(decision_rows=-1), dict(fic_group_tiles=65536),
                dict(gather_descs=65536), dict(gather_descs=-1), dict(fetch_words=-1), dict(fft_chunk_tfs=-5), dict(fft_chunk_tfs=(1 << 20) + 1)):
        with pytest.raises(dab.DabhipError, match="set_launch_limits"):
            eng.set_launch_limits(**bad)
        assert eng.decode([iq]) == len(want) and np.array_equal(eng.eti(0), want), bad
    with pytest.raises(ValueError):
        eng.set_launch_limits(no_such_limit=1)
    eng.set_launch_limits()                          # all defaults again
    assert eng.decode([iq]) == len(want) and np.array_equal(eng.eti(0), want)
    _report(eng, "(f) after the refusals, default limits", decoder=1, regroup=1, fic_group=1, fetch_form=dab.FETCH_KERNEL)
    eng.close()
    st = dab.Stream(1)
    with pytest.raises(dab.DabhipError, match="set_launch_limits"):
        st.set_launch_limits(gather_descs=70000)
    st.close()
    d = dab.Dab(0)
    with pytest.raises(dab.DabhipError, match="set_launch_limits"):
        d.set_launch_limits(regroup_tiles=9)
    d.close()
