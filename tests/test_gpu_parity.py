"""GPU parity tests: every stage of the HIP path, called through the C ABI, against the CPU
oracle on identical seeded inputs.  Bit-exact for bits, bytes and indices; the OFDM spectra
(fp32 on the GPU, fp64 in the oracle / FFTW in the reference) within a stated tolerance."""
import ctypes as C

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


def _noisy_codewords(rng, nbits, n, p_erase, p_flip):
    syms, datas = [], []
    for _ in range(n):
        d = rng.integers(0, 256, nbits // 8, dtype=np.uint8)
        s = 127 + 2 * ol.or_encode(d).astype(np.int32)
        flip = rng.random(s.size) < p_flip
        s = np.where(flip, 256 - s, s).astype(np.uint8)
        s[rng.random(s.size) < p_erase] = 128
        syms.append(s)
        datas.append(d)
    return np.concatenate(syms), datas


@pytest.mark.parametrize("nbits,n,p_erase,p_flip", [(768, 1, 0.0, 0.0), (768, 70, 0.25, 0.05), (192, 130, 0.5, 0.1),
                                                    (3072, 64, 0.3, 0.12), (9216, 3, 0.4, 0.08), (32, 5, 0.0, 0.2)])
def test_viterbi_matches_scalar_reference_decisions(nbits, n, p_erase, p_flip):
    rng = np.random.default_rng(nbits + n)
    sym, _ = _noisy_codewords(rng, nbits, n, p_erase, p_flip)
    got = dab.viterbi(sym, nbits, n)
    per = 4 * (nbits + 6)
    for i in range(n):
        want = ol.or_viterbi(sym[i * per:(i + 1) * per], nbits)
        assert np.array_equal(got[i], want), "code word %d" % i


def test_viterbi_all_erased_and_ties():
    # all symbols erased: every compare is a tie -> the low predecessor everywhere -> all-zero data
    nbits = 768
    sym = np.full(4 * (nbits + 6), 128, dtype=np.uint8)
    assert not dab.viterbi(sym, nbits, 1).any()
    # half-erased alternating pattern produces many exact ties
    sym[::2] = 127
    sym[1::8] = 129
    assert np.array_equal(dab.viterbi(sym, nbits, 1)[0], ol.or_viterbi(sym, nbits))


def _aligned_frames(ntf, seed, snr_db=1000.0):
    cfg = dab.synth_preset(1, seed=seed, snr_db=snr_db)
    iq = dab.synth_generate(cfg, ntf)
    return iq.reshape(ntf, dab.TF_BYTES)


def _oracle_symbols(frame):
    """fp64 fftshifted spectra of one aligned frame via the oracle's DFT."""
    O = ol.oracle()
    x = frame.astype(np.int32) - 127
    x = ((x + 128) & 255) - 128            # int8 wrap, input_sdr.c:61-62
    x = x.astype(np.float64).reshape(-1, 2)
    out = np.zeros((76, 2048, 2))
    tmp = np.zeros((2048, 2))
    for i in range(76):
        w = np.ascontiguousarray(x[2656 + 2552 * i + 504: 2656 + 2552 * i + 504 + 2048])
        O.or_dft(2048, w.ctypes.data_as(C.POINTER(C.c_double)), tmp.ctypes.data_as(C.POINTER(C.c_double)), -1)
        out[i] = np.roll(tmp, 1024, axis=0)
    return out


def test_ofdm_fft_vs_fp64_dft(engine):
    frames = _aligned_frames(2, seed=5, snr_db=15.0)
    got, _ = engine.stage_ofdm_fft(frames)
    for f in range(2):
        want = _oracle_symbols(frames[f])
        scale = np.abs(want).max()
        err = np.abs(got[f].astype(np.float64) - want).max() / scale
        # fp32 radix-8 transform of +-128 integers vs the fp64 DFT: tolerance 2e-6 of full scale
        assert err < 2e-6, err
        # ... and against numpy.fft (pocketfft, fp64), which shares no code with the oracle: same tolerance
        x = frames[f].astype(np.int32) - 127
        x = (((x + 128) & 255) - 128).astype(np.float64).reshape(-1, 2)
        z = x[:, 0] + 1j * x[:, 1]
        ref = np.stack([np.fft.fftshift(np.fft.fft(z[2656 + 2552 * i + 504: 2656 + 2552 * i + 504 + 2048])) for i in range(76)])
        got_c = got[f][..., 0].astype(np.float64) + 1j * got[f][..., 1].astype(np.float64)
        assert np.abs(got_c - ref).max() / np.abs(ref).max() < 2e-6


def test_demap_bits_match_oracle(engine):
    """K2 + K2b give the same 230,400 hard bits per TF as the oracle's fp64 front end."""
    cfg = dab.synth_preset(1, seed=9, snr_db=12.0)
    iq = dab.synth_generate(cfg, 6)
    O = ol.oracle()
    S = O.or_sdr_new()
    fic = np.zeros(dab.FIC_BITS, np.uint8)
    msc = np.zeros(dab.MSC_BITS, np.uint8)
    checked = 0
    for off in range(0, iq.size - dab.CHUNK_BYTES + 1, dab.CHUNK_BYTES):
        ch = iq[off:off + dab.CHUNK_BYTES]
        if O.or_sdr_demod(S, ol._ptr(ch), dab.CHUNK_BYTES, ol._ptr(fic), ol._ptr(msc)):
            frame = np.ctypeslib.as_array(O.or_sdr_buffer(S), (dab.TF_BYTES,)).copy()
            spec, _ = engine.stage_ofdm_fft(frame)
            gfic, gmsc = engine.stage_demap(spec)
            assert np.array_equal(gfic[0], fic)
            assert np.array_equal(gmsc[0], msc)
            checked += 1
    O.or_sdr_free(S)
    assert checked >= 2


def test_fic_decode_matches_oracle(engine):
    rng = np.random.default_rng(3)
    cfg = dab.synth_preset(0, seed=4)
    O = ol.oracle()
    n = 5
    fic = np.zeros((n, dab.FIC_BITS), np.uint8)
    for t in range(n):
        for q in range(4):
            fibs = dab.synth_fibs(cfg, 4 * t + q)
            scr = fibs.copy()
            O.or_descramble(ol._ptr(scr), 96)
            mother = ol.or_encode(scr)
            dep = np.zeros(3096, np.uint8)
            # puncture = positions the FIC depuncturer does not erase
            O.or_fic_depuncture(ol._ptr(dep), ol._ptr(np.zeros(2304, np.uint8)))
            fic[t, 2304 * q:2304 * (q + 1)] = mother[dep != 128]
    fic[1, rng.integers(0, dab.FIC_BITS, 300)] ^= 1      # correctable
    fic[3, rng.integers(0, dab.FIC_BITS, 2500)] ^= 1     # not correctable: CRC failures
    fibs, ok = engine.stage_fic_decode(fic)
    for t in range(n):
        wf = np.zeros((12, 32), np.uint8)
        wo = np.zeros(12, np.uint8)
        O.or_fic_decode(ol._ptr(fic[t]), ol._ptr(wf), ol._ptr(wo))
        assert np.array_equal(fibs[t], wf) and np.array_equal(ok[t], wo), t
    assert ok[0].all() and ok[1].all() and not ok[3].all()


def _check_streams(engine, streams):
    total = engine.decode(streams)
    n = 0
    for b, iq in enumerate(streams):
        want, trace = ol.or_replay(iq)
        got = engine.eti(b)
        assert got.shape == want.shape, (b, got.shape, want.shape)
        assert np.array_equal(got, want), "stream %d ETI bytes differ" % b
        ints, ffs = engine.trace(b, len(trace))
        for k, t in enumerate(trace):
            assert tuple(ints[k]) == (t.ok, t.read_frame, t.coarse_timeshift, t.fine_timeshift, t.coarse_freq_shift, t.fifo_count), (b, k)
            # fine frequency estimate: fp64 atan2 sum, different summation order -> 1e-9 Hz
            assert abs(ffs[k] - t.fine_freq_shift) < 1e-9
        n += len(want)
    assert total == n
    return n


def test_engine_e2e_clean_aligned_and_offset(engine):
    streams = []
    for seed, skip, preset in ((21, 0, 1), (22, 50000, 1), (23, 123457, 0), (24, 196000, 1)):
        cfg = dab.synth_preset(preset, seed=seed, cif_count0=(37 * seed) % 5000, skip_samples=skip)
        streams.append(dab.synth_generate(cfg, 22))
    assert _check_streams(engine, streams) >= 4 * 20


def test_engine_e2e_noisy_and_ragged(engine):
    streams = []
    for seed, snr, ntf in ((31, 14.0, 24), (32, 9.0, 30), (33, 7.0, 26), (34, 1000.0, 3), (35, 1000.0, 17)):
        cfg = dab.synth_preset(1, seed=seed, snr_db=snr, cif_count0=4990)
        iq = dab.synth_generate(cfg, ntf)
        streams.append(iq[: iq.size - 1000 * seed])       # ragged: trailing partial chunk is dropped
    _check_streams(engine, streams)


def test_engine_payload_roundtrip(engine):
    """encode -> modulate -> demodulate -> decode returns the payload that was sent."""
    cfg = dab.synth_preset(0, seed=77, cif_count0=1234)
    iq = dab.synth_generate(cfg, 19)
    assert engine.decode([iq]) == 16
    eti = engine.eti(0)
    for f in range(16):
        e = eti[f].astype(int)
        nst = e[5] & 0x7f
        assert nst == 12
        pos = 12 + 4 * nst
        cif = 40 + f                                  # first emitted frame = first CIF of the 10th good TF
        assert np.array_equal(eti[f][pos:pos + 96], dab.synth_fibs(cfg, cif))
        pos += 96
        for k in range(nst):
            stl = ((e[8 + 4 * k + 2] & 3) << 8) | e[8 + 4 * k + 3]
            want = dab.synth_payload(cfg, cif, k)
            assert stl * 8 == want.size
            assert np.array_equal(eti[f][pos:pos + want.size], want), (f, k)
            pos += want.size


def test_seams_s2_s3_streaming_match_oracle():
    """The single-stream seams (sdr_demod, dab_process_frame) driven like dab2eti.c:60-130."""
    cfg = dab.synth_preset(1, seed=41, skip_samples=77777, snr_db=11.0)
    iq = dab.synth_generate(cfg, 24)
    want, trace = ol.or_replay(iq)
    sdr, d = dab.Sdr(0), dab.Dab(0)
    k = 0
    for off in range(0, iq.size - dab.CHUNK_BYTES + 1, dab.CHUNK_BYTES):
        ok = sdr.demod(iq[off:off + dab.CHUNK_BYTES])
        t = trace[k]
        assert ok == t.ok
        assert sdr.state[:3] == (t.coarse_timeshift, t.fine_timeshift, t.coarse_freq_shift), k
        if ok:
            d.fic[:] = sdr.fic
            d.msc[:] = sdr.msc
            d.process_frame()
        k += 1
    got = np.array(d.frames)
    assert got.shape == want.shape and np.array_equal(got, want)
    sdr.close()
    d.close()


def test_seam_s3_against_real_reference_backend():
    """dab_process_frame fed with demapped bits: HIP back end vs the REAL reference objects."""
    R = ol.ref()
    if R is None:
        pytest.skip("oracle/_ref not built")
    cfg = dab.synth_preset(0, seed=51, snr_db=8.5)
    iq = dab.synth_generate(cfg, 21)
    O = ol.oracle()
    S = O.or_sdr_new()
    H = R.refh_new()
    d = dab.Dab(0)
    fic = np.zeros(dab.FIC_BITS, np.uint8)
    msc = np.zeros(dab.MSC_BITS, np.uint8)
    for off in range(0, iq.size - dab.CHUNK_BYTES + 1, dab.CHUNK_BYTES):
        ch = iq[off:off + dab.CHUNK_BYTES]
        if O.or_sdr_demod(S, ol._ptr(ch), dab.CHUNK_BYTES, ol._ptr(fic), ol._ptr(msc)):
            C.memmove(R.refh_tf_fic(H), ol._ptr(fic), fic.size)
            C.memmove(R.refh_tf_msc(H), ol._ptr(msc), msc.size)
            R.refh_process(H)
            d.fic[:] = fic
            d.msc[:] = msc
            d.process_frame()
    n = R.refh_neti(H)
    want = np.ctypeslib.as_array(R.refh_eti(H), (n, 6144)).copy() if n else np.zeros((0, 6144), np.uint8)
    got = np.array(d.frames).reshape(-1, 6144)
    assert n > 0 and got.shape == want.shape and np.array_equal(got, want)
    O.or_sdr_free(S)
    d.close()


def test_seam_s3_golden_reference_eti():
    """Committed golden fixture: demapped bits of 32 TFs (9 dB SNR, one lock loss) -> the ETI bytes
    the real reference produced (tests/golden/make_golden.py)."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backend_e2e.npz"))
    d = dab.Dab(0)
    for row in g["tf_bits"]:
        bits = np.unpackbits(row)
        d.fic[:] = bits[:9216]
        d.msc[:] = bits[9216:]
        d.process_frame()
    got = np.array(d.frames)
    assert got.shape == g["eti"].shape and np.array_equal(got, g["eti"])
    d.close()


def test_viterbi_golden_known_answers():
    import os
    kat = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backend_kat.npz"))
    for i in range(int(kat["vit_count"])):
        sym, want = kat["vit%d_sym" % i], kat["vit%d_out" % i]
        assert np.array_equal(dab.viterbi(sym, want.size * 8, 1)[0], want), i


def test_s3_long_run_slot_recycling():
    """More TFs than the seam's 64 device slots: the slot window is recycled without changing the output."""
    cfg = dab.synth_preset(1, seed=61)
    iq = dab.synth_generate(cfg, 85)
    want, _ = ol.or_replay(iq)
    sdr, d = dab.Sdr(0), dab.Dab(0)
    for off in range(0, iq.size - dab.CHUNK_BYTES + 1, dab.CHUNK_BYTES):
        if sdr.demod(iq[off:off + dab.CHUNK_BYTES]):
            d.fic[:] = sdr.fic
            d.msc[:] = sdr.msc
            d.process_frame()
    got = np.array(d.frames)
    assert len(want) == 4 * (85 - 15) and got.shape == want.shape and np.array_equal(got, want)
    sdr.close()
    d.close()


def test_cli_stdout_contract(tmp_path):
    """dab2eti-hip file.cu8 > out.eti : 6144-byte frames on stdout, identical to the oracle replay, file by file."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(dab.LIB_PATH), "dab2eti-hip")
    assert os.path.exists(exe), "dab2eti-hip not built"
    files, want = [], []
    for i, (seed, skip) in enumerate(((71, 0), (72, 4242))):
        iq = dab.synth_generate(dab.synth_preset(1, seed=seed, skip_samples=skip), 20)
        path = tmp_path / ("cap%d.cu8" % i)
        iq.tofile(path)
        files.append(str(path))
        want.append(ol.or_replay(iq)[0])
    out = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout
    got = np.frombuffer(out, dtype=np.uint8).reshape(-1, 6144)
    assert np.array_equal(got, np.concatenate(want))
    # streaming mode: stdin, small segments, bounded memory -- the same bytes
    with open(files[1], "rb") as f:
        out = subprocess.run([exe, "--segment-calls", "5", "-"], stdin=f, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout
    assert np.array_equal(np.frombuffer(out, dtype=np.uint8).reshape(-1, 6144), want[1])
    out = subprocess.run([exe, "--stream", files[0]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout
    assert np.array_equal(np.frombuffer(out, dtype=np.uint8).reshape(-1, 6144), want[0])


def test_engine_e2e_low_snr_lock_loss(engine):
    """5-6 dB SNR (BASELINE config 5 regime): hard decisions fail, FIBs break, lock is lost and regained;
    the HIP path must still reproduce the reference semantics byte for byte (scalar viterbi.c decisions)."""
    streams = []
    for seed, snr in ((81, 6.0), (82, 5.0), (83, 5.5)):
        streams.append(dab.synth_generate(dab.synth_preset(1, seed=seed, snr_db=snr), 40))
    total = engine.decode(streams)
    unlocked = 0
    for b, iq in enumerate(streams):
        want, trace = ol.or_replay(iq)
        got = engine.eti(b)
        assert got.shape == want.shape and np.array_equal(got, want), b
        ints, _ = engine.trace(b, len(trace))
        assert [tuple(r[:5]) for r in ints] == [(t.ok, t.read_frame, t.coarse_timeshift, t.fine_timeshift, t.coarse_freq_shift) for t in trace]
        unlocked += int(len(want) < 4 * (40 - 15))
    assert unlocked >= 1          # at least one stream actually lost frames at this SNR


def test_engine_edge_inputs(engine):
    """Ragged / degenerate inputs: shorter than one call, no signal at all, clipped full-scale noise, a stream that
    ends right after lock.  Traces and (empty or short) ETI outputs must equal the oracle's."""
    rng = np.random.default_rng(5)
    good = dab.synth_generate(dab.synth_preset(1, seed=91), 16)            # exactly 4 ETI frames
    streams = [
        np.full(100000, 127, np.uint8),                                     # < one 262144-byte call: nothing happens
        np.full(3 * dab.TF_BYTES, 127, np.uint8),                           # silence: in "sync", FIBs never pass
        rng.integers(0, 256, 4 * dab.TF_BYTES, dtype=np.uint8),             # full-scale noise incl. 255 -> int8 wrap
        good,
        good[: 14 * dab.TF_BYTES],                                          # ends before the first frame is due
        np.concatenate([good[:5 * dab.TF_BYTES], rng.integers(100, 156, 2 * dab.TF_BYTES, dtype=np.uint8), good[5 * dab.TF_BYTES:]]),
    ]
    total = engine.decode(streams)
    n = 0
    for b, iq in enumerate(streams):
        want, trace = ol.or_replay(iq)
        got = engine.eti(b)
        assert got.shape == want.shape and np.array_equal(got, want), b
        ints, _ = engine.trace(b, max(len(trace), 1))
        for k, t in enumerate(trace):
            assert tuple(ints[k]) == (t.ok, t.read_frame, t.coarse_timeshift, t.fine_timeshift, t.coarse_freq_shift, t.fifo_count), (b, k)
        n += len(want)
    assert total == n and engine.eti_count(3) == 4 and engine.eti_count(0) == 0


def test_engine_many_subchannels_and_uep_eep_mix(engine):
    """A dense custom multiplex: 20 sub-channels incl. the smallest and largest code words the tables allow here."""
    cfg = dab.synth_preset(0, seed=95)
    cfg.nsub = 0
    cu = 0
    def add(slform, idx_or_lev, size=0):
        nonlocal cu
        k = cfg.nsub
        cfg.sub[k].id = 3 * k + 1
        cfg.sub[k].start_cu = cu
        cfg.sub[k].slform = slform
        if slform == 0:
            cfg.sub[k].uep_index = idx_or_lev
            cu += [16, 21, 24, 29, 35, 24, 29, 35, 42, 52, 29, 35, 42, 52, 32, 42, 48, 58, 70, 40][idx_or_lev] if idx_or_lev < 20 else 0
        else:
            cfg.sub[k].eep_protlev = idx_or_lev
            cfg.sub[k].size_cu = size
            cu += size
        cfg.nsub += 1
    for idx in (0, 4, 5, 9, 14, 18):       # UEP 32k PL5, 32k PL1, 48k PL5, 48k PL1, 64k PL5, 64k PL1
        add(0, idx)
    for lev, size in ((0, 12), (1, 8), (2, 6), (3, 4), (4, 27), (5, 21), (6, 18), (7, 15), (0, 96), (3, 64), (1, 16), (2, 12), (3, 8), (7, 30)):
        add(1, lev, size)
    assert cfg.nsub == 20 and cu <= 864
    iq = dab.synth_generate(cfg, 18)
    assert engine.decode([iq]) == 12
    want, _ = ol.or_replay(iq)
    got = engine.eti(0)
    assert np.array_equal(got, want)
    e = got[0].astype(int)
    assert (e[5] & 0x7f) == 20


def test_full_size_batch_properties():
    """BASELINE configs[2] size (256 streams x 64 TF, 12 sub-channels): size-independent properties.
    (a) every ETI frame of sampled streams is well formed (HCRC, EOF CRC, FL, FSYNC/FCT, padding);
    (b) encode -> modulate -> decode returns the payload;  (c) identical inputs give identical outputs;
    (d) one stream is compared byte for byte with the CPU oracle."""
    import eti_check
    ntf, distinct, nstreams = 64, 8, 256
    cfgs = [dab.synth_preset(0, seed=300 + i, cif_count0=(611 * i) % 5000) for i in range(distinct)]
    host = [dab.synth_generate(c, ntf) for c in cfgs]
    tensors = []
    for i in range(nstreams):                                    # device memory through the library itself (no second GPU runtime in the process)
        buf = dab.DeviceBuffer(host[i % distinct].size)
        buf.upload(host[i % distinct])
        tensors.append(buf)
    eng = dab.Engine(0)
    total = eng.decode_device([t.ptr for t in tensors], [t.nbytes for t in tensors])
    assert total == nstreams * 4 * (ntf - 15)
    ref = {}
    for b in list(range(distinct)) + [distinct + 3, 100, 255]:
        eti = eng.eti(b)
        assert eti.shape == (4 * (ntf - 15), 6144)
        if b < distinct:
            ref[b] = eti
            assert eti_check.check_sequence(eti) == 196                       # (a)
            for f in (0, 77, 195):                                            # (b)
                p = eti_check.parse(eti[f])
                cif = 40 + f
                assert np.array_equal(p["fic"], dab.synth_fibs(cfgs[b], cif))
                for k, data in enumerate(p["subch"]):
                    assert np.array_equal(data, dab.synth_payload(cfgs[b], cif, k)), (b, f, k)
        else:
            assert np.array_equal(eti, ref[b % distinct])                     # (c)
    want, _ = ol.or_replay(host[5])                                           # (d)
    assert np.array_equal(ref[5], want)
    eng.close()


def test_software_afc_decodes_offset_captures():
    """SURVEY 8(f) rank 1 (beyond the reference, which needs a tuner): with the NCO steered by the reference's AFC rule,
    captures with a carrier offset lock and return the transmitted payload; in parity mode (default) large offsets
    never lock, exactly like the reference without its tuner."""
    import eti_check
    ntf = 70
    cfgs = [dab.synth_preset(1, seed=400 + i, cfo_hz=cfo, snr_db=20.0) for i, cfo in enumerate((3400.0, -1700.0, 260.0, 0.0))]
    streams = [dab.synth_generate(c, ntf) for c in cfgs]
    eng = dab.Engine(0)
    eng.decode(streams)
    assert eng.eti_count(0) == 0 and eng.eti_count(1) == 0            # parity mode: > 1 carrier off -> never demodulated
    assert eng.eti_count(3) == 4 * (ntf - 15)
    eng.set_afc(True)
    eng.decode(streams)
    for b, cfg in enumerate(cfgs):
        eti = eng.eti(b)
        assert len(eti) >= 4 * (ntf - 15) - 4 * 14, (b, len(eti))      # at most a few TFs spent pulling in
        ints, ffs = eng.trace(b, 3 * ntf // 2)
        assert abs(ffs[len(ints) - 1]) < 60.0                         # residual offset inside the rule's dead band
        # frames are well formed and carry the payload of the CIF their FIC announces
        for f in (0, len(eti) // 2, len(eti) - 1):
            p = eti_check.parse(eti[f])
            cif = next(c for c in range(4 * ntf) if np.array_equal(dab.synth_fibs(cfg, c), p["fic"]))
            for k, data in enumerate(p["subch"]):
                assert np.array_equal(data, dab.synth_payload(cfg, cif, k)), (b, f, k)
    eng.close()


def test_software_afc_trace_equals_the_oracles_tuner_rule():
    """the AFC is trace-checked, not only property-checked.  or_replay_afc restates the tuner feedback of demod_thread_fn
    (dab2eti.c:76-103: |coarse| > 1 -> -+1000 Hz, == 1 -> a random step below 1 kHz, else fine / 3 beyond 50 Hz, after EVERY call) on an fp64 NCO;
    call by call the GPU's re-tuning sequence, the integer shifts, the call at which each frame is accepted and the ETI bytes are the oracle's.
    (The frequency estimate is compared to 1e-6 Hz: K1 de-rotates in fp64 like the oracle.)"""
    ntf = 40
    cfgs = [dab.synth_preset(1, seed=450 + i, cif_count0=77 * i, cfo_hz=cfo, snr_db=snr, skip_samples=skip)
            for i, (cfo, snr, skip) in enumerate(((3400.0, 25.0, 0), (-1700.0, 25.0, 30000), (1100.0, 1000.0, 0), (-260.0, 15.0, 0), (0.0, 1000.0, 0)))]
    streams = [dab.synth_generate(c, ntf) for c in cfgs]
    eng = dab.Engine(0)
    eng.set_afc(True)
    eng.decode(streams)
    for b, iq in enumerate(streams):
        want_eti, want_tr, want_nco = ol.or_replay_afc(iq)
        ints, ffs = eng.trace(b, len(want_tr))
        nco = eng.trace_nco(b, len(want_tr))
        assert len(ints) == len(want_tr)
        assert np.array_equal(nco, want_nco), (b, list(nco[:30]), list(want_nco[:30]))
        for k, t in enumerate(want_tr):
            assert tuple(ints[k][:5]) == (t.ok, t.read_frame, t.coarse_timeshift, t.fine_timeshift, t.coarse_freq_shift), (b, k)
            assert ints[k][5] == t.fifo_count and abs(ffs[k] - t.fine_freq_shift) < 1e-6, (b, k, ffs[k], t.fine_freq_shift)
        if b < 4:
            assert len(set(want_nco.tolist())) > 2                      # the rule did move the NCO
        assert np.array_equal(eng.eti(b), want_eti), "stream %d: ETI differs from the oracle's AFC replay" % b
    eng.close()


def _payload_errors(eti, cfg, ntf):
    """(frames, frames whose MST differs from what was sent, wrong payload bits, payload bits) over the decoded frames"""
    import eti_check
    frames = bad = werr = bits = 0
    for e in eti:
        try:
            p = eti_check.parse(e)
        except AssertionError:
            frames += 1
            bad += 1
            continue
        cif = next((c for c in range(4 * ntf) if np.array_equal(dab.synth_fibs(cfg, c), p["fic"])), None)
        frames += 1
        if cif is None:
            bad += 1
            continue
        wrong = 0
        for k, data in enumerate(p["subch"]):
            want = dab.synth_payload(cfg, cif, k)
            wrong += int(np.unpackbits(np.bitwise_xor(data, want)).sum())
            bits += 8 * want.size
        werr += wrong
        bad += int(wrong > 0)
    return frames, bad, werr, bits


def test_soft_decision_mode():
    """SURVEY 8(f) rank 2 / BASELINE config 5 (extension: the reference has hard decisions only).
    (a) clean and 20 dB input: soft decoding returns exactly the bytes of the reference semantics;
    (b) 6.0 - 7.5 dB SNR: soft decoding delivers more frames and fewer payload bit errors than hard decoding."""
    ntf = 40
    eng = dab.Engine(0)
    eng.set_soft(True)
    clean = [dab.synth_generate(dab.synth_preset(1, seed=500 + i, snr_db=snr, skip_samples=sk), 24) for i, (snr, sk) in enumerate(((1000.0, 0), (20.0, 31000)))]
    eng.decode(clean)
    for b, iq in enumerate(clean):
        want, _ = ol.or_replay(iq)
        assert np.array_equal(eng.eti(b), want), b                     # (a)
    cfgs = [dab.synth_preset(1, seed=510 + i, snr_db=snr) for i, snr in enumerate((7.5, 7.0, 6.5, 6.0))]
    noisy = [dab.synth_generate(c, ntf) for c in cfgs]
    eng.decode(noisy)
    soft = [_payload_errors(eng.eti(b), cfgs[b], ntf) for b in range(len(noisy))]
    eng.set_soft(False)
    eng.decode(noisy)
    hard = [_payload_errors(eng.eti(b), cfgs[b], ntf) for b in range(len(noisy))]
    good_soft = sum(f - bad for f, bad, _, _ in soft)
    good_hard = sum(f - bad for f, bad, _, _ in hard)
    print("error-free frames soft/hard:", good_soft, good_hard, "detail", soft, hard)
    assert good_soft > good_hard                                        # (b)
    assert sum(s[0] for s in soft) >= sum(h[0] for h in hard)          # soft FIC keeps lock at least as long
    eng.close()


@pytest.mark.gpu
def test_device_modulator_matches_host_generator_and_decodes():
    """the GPU modulator emits the host generator's signal (up to fp32-vs-fp64 rounding of a
    sample, one LSB) and what the engine decodes from it equals the oracle on the very same bytes."""
    ntf = 20
    cfgs = [dab.synth_preset(1, seed=7),
            dab.synth_preset(0, seed=8, cif_count0=4990, skip_samples=50001),
            dab.synth_preset(1, seed=9, snr_db=15.0, cfo_hz=130.0, amplitude=0.8)]
    bufs = [dab.DeviceBuffer(dab.synth_bytes(c, ntf)) for c in cfgs]
    dab.synth_generate_device(cfgs, ntf, [b.ptr for b in bufs])
    got = [b.download() for b in bufs]
    for c, g in zip(cfgs, got):
        want = dab.synth_generate(c, ntf)
        assert g.size == want.size
        diff = np.abs(g.astype(np.int16) - want.astype(np.int16))
        assert diff.max() <= 1
        assert (diff != 0).mean() < 2e-3
    eng = dab.Engine(0)
    eng.decode_device([b.ptr for b in bufs], [b.nbytes for b in bufs])
    for i, g in enumerate(got):
        want, _ = ol.or_replay(g)
        assert np.array_equal(eng.eti(i), want)
    assert len(eng.eti(0)) == 4 * (ntf - 15)


@pytest.mark.gpu
@pytest.mark.parametrize("soft", [False, True])
def test_streaming_session_equals_one_shot_decode(soft):
    """captures fed to a session in segments of arbitrary size (not multiples of the 262144-byte
    call, ragged across streams, some empty) give, concatenated, the ETI frames of one decode of the whole captures --
    for an aligned stream, a mid-frame start, a noisy one that loses lock, and one with a coarse resync."""
    ntf = 34
    cfgs = [dab.synth_preset(1, seed=21), dab.synth_preset(0, seed=22, skip_samples=77777, cif_count0=4995),
            dab.synth_preset(1, seed=23, snr_db=7.5), dab.synth_preset(1, seed=24, skip_samples=150001)]
    caps = [dab.synth_generate(c, ntf) for c in cfgs]
    caps[3] = np.concatenate([caps[3][:9 * 393216 + 1000], caps[3][9 * 393216 + 61000:]])   # 30000 samples vanish: coarse resync
    eng = dab.Engine(0)
    eng.set_soft(soft)
    eng.decode(caps)
    want = [eng.eti(i) for i in range(len(caps))]
    assert len(want[0]) == 4 * (ntf - 15) and len(want[3]) > 0
    if not soft:
        for c, w in zip(caps, want):
            assert np.array_equal(w, ol.or_replay(c)[0])
    rng = np.random.default_rng(5)
    for trial, sizes in enumerate([[262144 * 12] * 4, [1000003, 3 * 262144, 5000000, 262144 * 7 + 2], None]):
        st = dab.Stream(len(caps), soft=soft)
        pos = [0] * len(caps)
        got = [[] for _ in caps]
        nseg = 0
        while any(p < c.size for p, c in zip(pos, caps)):
            segs = []
            for b, c in enumerate(caps):
                n = sizes[b] if sizes else int(rng.choice([0, 2, 300000, 262144 * 3, 393216 * 5 + 6, 4000000]))
                n -= n & 1
                segs.append(c[pos[b]:pos[b] + n])
                pos[b] += segs[-1].size
            total = st.feed(segs)
            nseg += 1
            per = [st.eti(b) for b in range(len(caps))]
            assert total == sum(len(p) for p in per)
            for b, p in enumerate(per):
                got[b].append(p)
        assert nseg > 3
        for b in range(len(caps)):
            assert np.array_equal(np.concatenate(got[b]), want[b]), "trial %d stream %d" % (trial, b)
        st.close()


@pytest.mark.gpu
def test_fused_and_two_kernel_ofdm_stages_give_identical_frames():
    """The one-kernel OFDM stage (k_fused.hip, spectra never written; the default) against K2 + K2b: identical ETI on clean,
    unaligned, noisy (lock loss) and resynchronising captures, with and without the software AFC -- and, AFC off, both
    equal to the CPU oracle on every stream."""
    ntf = 24
    cfgs = [dab.synth_preset(0, seed=31), dab.synth_preset(1, seed=32, skip_samples=123457), dab.synth_preset(1, seed=33, snr_db=6.5),
            dab.synth_preset(0, seed=34, snr_db=9.0, cif_count0=4990), dab.synth_preset(1, seed=35, cfo_hz=-1700.0)]
    caps = [dab.synth_generate(c, ntf) for c in cfgs]
    caps.append(np.concatenate([caps[0][:7 * 393216], caps[0][7 * 393216 + 50000:]]))
    for afc in (False, True):
        eng = dab.Engine(0)
        eng.set_afc(afc)
        eng.set_fused(False)
        eng.decode(caps)
        want = [eng.eti(i) for i in range(len(caps))]
        flagged_two = eng.guard_stats()[0]
        eng.set_fused(True)
        eng.decode(caps)
        flagged_fused = eng.guard_stats()[0]
        if afc:
            assert flagged_two == flagged_fused == 0            # no parity guard with the NCO in the path
        else:                                                   # both stages list (almost) the same decisions for the fp64 re-decision
            assert flagged_two > 0 and abs(flagged_fused - flagged_two) <= 2 + flagged_two // 100
        for i in range(len(caps)):
            assert np.array_equal(eng.eti(i), want[i]), "stream %d afc %d" % (i, afc)
        assert sum(len(w) for w in want) > 100
        if not afc:
            for i, c in enumerate(caps):
                assert np.array_equal(want[i], ol.or_replay(c)[0]), i
        eng.close()


@pytest.mark.gpu
def test_streaming_session_carries_the_afc_state():
    """The NCO frequency and the tuner rule's generator live in the carried front-end state: an offset capture decodes
    the same whether it is fed at once or in segments, and the CLI's --afc reaches both modes."""
    import os
    import subprocess
    import tempfile
    cap = dab.synth_generate(dab.synth_preset(1, seed=41, cfo_hz=2600.0), 44)
    eng = dab.Engine(0)
    eng.set_afc(True)
    eng.decode([cap])
    want = eng.eti(0)
    assert len(want) > 60                     # locks after the NCO has pulled in
    st = dab.Stream(1, afc=True)
    got, pos = [], 0
    for n in (262144 * 9, 1234568, 262144 * 30, 5000000, 10 ** 9):
        st.feed([cap[pos:pos + n]])
        got.append(st.eti(0))
        pos += n
    assert np.array_equal(np.concatenate(got), want)
    st.close()
    exe = os.path.join(os.path.dirname(dab.LIB_PATH), "dab2eti-hip")
    with tempfile.NamedTemporaryFile(suffix=".cu8") as f:
        cap.tofile(f.name)
        out = subprocess.run([exe, "--afc", "--segment-calls", "11", "--stream", f.name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout
    assert np.array_equal(np.frombuffer(out, dtype=np.uint8).reshape(-1, 6144), want)


@pytest.mark.gpu
def test_engine_reuse_across_batch_shapes_and_modes():
    """One engine, decodes of different shapes and modes back to back (grow-only buffers, reused work lists, persistent
    session state must not leak from one call into the next): every result equals that of a fresh engine."""
    a = [dab.synth_generate(dab.synth_preset(0, seed=51 + i, skip_samples=1000 * i), 22) for i in range(5)]
    b = [dab.synth_generate(dab.synth_preset(1, seed=61, snr_db=8.0), 30)]
    c = [dab.synth_generate(dab.synth_preset(1, seed=62), 17), np.zeros(0, np.uint8), dab.synth_generate(dab.synth_preset(1, seed=63), 3)]

    def fresh(caps, **kw):
        e = dab.Engine(0)
        for k, v in kw.items():
            getattr(e, "set_" + k)(v)
        e.decode(caps)
        return [e.eti(i) for i in range(len(caps))]

    want_a, want_b, want_c = fresh(a), fresh(b), fresh(c)
    want_b_soft, want_a_fused = fresh(b, soft=True), fresh(a, fused=True)
    eng = dab.Engine(0)
    for caps, want, mode in ((a, want_a, {}), (b, want_b, {}), (c, want_c, {}), (b, want_b_soft, {"soft": True}), (a, want_a, {"soft": False}),
                             (a, want_a_fused, {"fused": True}), (c, want_c, {"fused": False}), (a, want_a, {})):
        for k, v in mode.items():
            getattr(eng, "set_" + k)(v)
        eng.decode(caps)
        for i, w in enumerate(want):
            assert np.array_equal(eng.eti(i), w)
    st = dab.Stream(1)                                    # a session after one-shot decodes on the same device
    st.feed([b[0][:5000000]])
    first = st.eti(0)
    st.feed([b[0][5000000:]])
    assert np.array_equal(np.concatenate([first, st.eti(0)]), want_b[0])
    assert all(np.array_equal(x, y) for x, y in zip(want_a, want_a_fused))


@pytest.mark.gpu
def test_subchannel_filter_carries_exactly_the_selected_payload():
    """TODO.md:28-31: with a sub-channel filter the frames list only the chosen SubChIds (valid header, FL, CRCs), each
    payload byte-identical to the unfiltered frame's, the FIC untouched; an empty list restores the reference's frames."""
    import eti_check
    cap = dab.synth_generate(dab.synth_preset(0, seed=71, cif_count0=123), 20)
    eng = dab.Engine(0)
    eng.decode([cap])
    full = eng.eti(0)
    assert len(full) == 20 and np.array_equal(full, ol.or_replay(cap)[0])
    eng.set_subchannels([5, 9, 40])                      # 40 is not in the ensemble
    eng.decode([cap])
    part = eng.eti(0)
    assert len(part) == len(full)
    import eti_filter_model
    assert np.array_equal(part, eti_filter_model.filter_frames(ol.or_replay(cap)[0], [5, 9, 40]))       # whole frames: the rewrite of the reference's
    for f, p in zip(full, part):
        a, b = eti_check.parse(f), eti_check.parse(p)
        assert [s[0] for s in b["stc"]] == [5, 9] and b["fct"] == a["fct"] and np.array_equal(a["fic"], b["fic"])
        for entry, payload in zip(b["stc"], b["subch"]):
            i = [s[0] for s in a["stc"]].index(entry[0])
            assert a["stc"][i] == entry and np.array_equal(a["subch"][i], payload)
    st = dab.Stream(1, subchannels=[5, 9])
    st.feed([cap[:3000000]])
    first = st.eti(0)
    st.feed([cap[3000000:]])
    assert np.array_equal(np.concatenate([first, st.eti(0)]), part)
    eng.set_subchannels([])
    eng.decode([cap])
    assert np.array_equal(eng.eti(0), full)


@pytest.mark.gpu
def test_whole_path_small_golden_on_gpu():
    """The committed whole-path fixture (tests/golden/e2e_small.npz: ETI bytes out of the real reference back end) against
    the batch engine, clean and at 10 dB with a mid-frame start."""
    import test_oracle_golden as tg
    caps, wants = [], []
    for ci, iq, same, want in tg._e2e_small_cases():
        if same:
            caps.append(iq)
            wants.append(want)
    assert caps, "no capture matched its recorded SHA-256"
    eng = dab.Engine(0)
    eng.decode(caps)
    for i, w in enumerate(wants):
        assert np.array_equal(eng.eti(i), w)
