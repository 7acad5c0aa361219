"""DAB+ (ETSI TS 102 563) without a GPU: the CPU model's CRCs, RS(120,110) code and sync rule, and the synthetic modulator's DAB+ superframes
against the model's packing.  Both are written from the standard; they agree with each other, and no broadcast recording pins them further."""
import numpy as np
import pytest

import dabplus_model as m
import dabtools_amd as dab


def test_au_crc_check_value_and_fib_crc():
    assert m.au_crc(b"123456789") == 0xD64E                              # CRC-16/GENIBUS
    cfg = dab.synth_preset(0, seed=3)
    for cif in (0, 1, 77, 249):
        fibs = dab.synth_fibs(cfg, cif).reshape(3, 32)
        for fib in fibs:
            assert m.au_crc(fib[:30]) == (int(fib[30]) << 8 | int(fib[31]))


def test_generator_roots_and_codewords():
    assert len(m.GEN) == 11 and m.GEN[0] == 1
    for i in range(10):
        assert m.poly_eval(m.GEN, int(m.EXP[i])) == 0
    rng = np.random.default_rng(7)
    for _ in range(20):
        d = rng.integers(0, 256, 110).astype(np.uint8)
        assert not any(m.syndromes(np.concatenate([d, m.rs_encode(d)])))


def test_up_to_five_errors_are_corrected_anywhere():
    rng = np.random.default_rng(11)
    for trial in range(240):
        d = rng.integers(0, 256, 110).astype(np.uint8)
        cw = np.concatenate([d, m.rs_encode(d)])
        n = trial % 6
        pos = rng.choice(120, n, replace=False)
        if trial % 12 == 5:
            pos = np.arange(115, 120)                                     # parity positions only
        r = cw.copy()
        r[pos] ^= rng.integers(1, 256, len(pos)).astype(np.uint8)
        out, fixed = m.rs_decode(r)
        assert fixed == len(pos) and (out == cw).all()


def test_six_to_eight_errors_fail_or_land_within_distance_five():
    rng = np.random.default_rng(13)
    fails = 0
    for trial in range(120):
        d = rng.integers(0, 256, 110).astype(np.uint8)
        cw = np.concatenate([d, m.rs_encode(d)])
        pos = rng.choice(120, 6 + trial % 3, replace=False)
        r = cw.copy()
        r[pos] ^= rng.integers(1, 256, len(pos)).astype(np.uint8)
        out, fixed = m.rs_decode(r)
        if fixed < 0:
            fails += 1
            assert (out == r).all()
        else:
            assert 0 < int((out != r).sum()) <= 5 and not any(m.syndromes(out))
    assert fails > 60


def _cfg_with_rates(seed, rates):
    """One EEP 4-A sub-channel per rate (8 s kbit/s = 4 s CU), every slot DAB+."""
    cfg = dab.synth_preset(1, seed=seed)
    cfg.nsub = len(rates)
    cu = 0
    for k, s in enumerate(rates):
        cfg.sub[k].id, cfg.sub[k].start_cu, cfg.sub[k].slform, cfg.sub[k].uep_index, cfg.sub[k].eep_protlev, cfg.sub[k].size_cu = 20 + k, cu, 1, 0, 3, 4 * s
        cu += 4 * s
    cfg.dabplus_slots = (1 << len(rates)) - 1
    return cfg


def test_synth_superframes_equal_the_model_packing():
    rates = [1, 4, 11, 12, 24, 48, 72]
    seen = {s: set() for s in rates}
    seed = 1
    while any(len(v) < 4 for v in seen.values()):
        cfg = _cfg_with_rates(seed, rates)
        cfg.dabplus_phase = seed % 5
        for slot, s in enumerate(rates):
            for n in (-1, 2):
                u = dab.synth_dabplus_superframe(cfg, n, slot)
                assert u.size == 110 * s
                r = m.parse(u)
                assert r["fire_ok"] and r["layout_ok"] and r["crc_ok"] == (1 << r["num_aus"]) - 1
                aus = m.good_aus(u, r)
                packed = m.pack_superframe(aus, s, r["dac_rate"], r["sbr_flag"], r["aac_channel_mode"], r["ps_flag"], r["mpeg_surround_config"])
                assert (packed == u).all(), (seed, s)
                sent = np.concatenate([dab.synth_payload(cfg, cfg.dabplus_phase + 5 * n + k, slot) for k in range(5)])
                assert (m.protect(packed) == sent).all(), (seed, s)
                seen[s].add(r["num_aus"])
        seed += 1
        assert seed < 40
    assert all(v == {2, 3, 4, 6} for v in seen.values())


def test_synth_dabplus_is_off_by_default_and_refused_with_reconfigurations():
    cfg = dab.synth_preset(0, seed=9)
    assert cfg.dabplus_slots == 0 and cfg.dabplus_phase == 0
    plain = dab.synth_payload(cfg, 12, 3)
    cfg.dabplus_slots = 1 << 3
    assert not (dab.synth_payload(cfg, 12, 3) == plain).all()
    assert (dab.synth_payload(cfg, 12, 2) == dab.synth_payload(dab.synth_preset(0, seed=9), 12, 2)).all()
    with pytest.raises(dab.DabhipError):
        dab.synth_dabplus_superframe(cfg, 0, 2)                           # not a DAB+ slot
    cfg.set_reconf(0, 40, cfg.multiplex())
    with pytest.raises(dab.DabhipError, match="reconfiguration"):
        dab.synth_generate(cfg, 1)


def _stream(rng, s, nsf, fct0, scid=5, dac=1, sbr=0):
    """nsf superframes of one sub-channel as ETI frames (model packing, random AUs)."""
    n, start0 = m.AU_LAYOUT[(dac, sbr)]
    frames = []
    for k in range(nsf):
        cuts = np.sort(rng.choice(np.arange(start0 + 3, 110 * s - 2), n - 1, replace=False))
        while np.any(np.diff(np.concatenate([[start0], cuts, [110 * s]])) < 3) or (n > 1 and cuts[-1] > 4095):
            cuts = np.sort(rng.choice(np.arange(start0 + 3, min(110 * s - 2, 4095)), n - 1, replace=False))
        bounds = np.concatenate([[start0], cuts, [110 * s]])
        aus = [rng.integers(0, 256, int(bounds[i + 1] - bounds[i] - 2)).astype(np.uint8).tobytes() for i in range(n)]
        sf = m.protect(m.pack_superframe(aus, s, dac, sbr))
        for p in range(5):
            frames.append(m.eti_frame(fct0 + 5 * k + p, [(scid, sf[24 * s * p:24 * s * (p + 1)])]))
    return frames


def test_sync_model_gives_the_same_superframes_in_any_chunking():
    rng = np.random.default_rng(5)
    frames = _stream(rng, 4, 12, 17)[3:]
    del frames[22]                                                        # an FCT gap
    whole = m.SyncModel(5)
    want = [(f, s, raw.tobytes()) for f, s, raw in whole.push(frames)]
    assert len(want) >= 8 and whole.losses == 1
    for chunk in (1, 3, 7):
        sm, got = m.SyncModel(5), []
        for i in range(0, len(frames), chunk):
            got += [(f, s, raw.tobytes()) for f, s, raw in sm.push(frames[i:i + chunk])]
        assert got == want and sm.losses == whole.losses


def test_adts_header_fields():
    h = m.adts_header(300, 1, 1, 1)                                       # 24 kHz core, stereo
    assert h[0] == 0xFF and h[1] >> 4 == 0xF and (h[1] & 1) == 1         # sync word, no CRC
    assert h[2] >> 6 == 1 and (h[2] >> 2) & 15 == 6                      # AAC LC, sampling index 6
    assert ((h[2] & 1) << 2 | h[3] >> 6) == 2
    assert ((h[3] & 3) << 11 | h[4] << 3 | h[5] >> 5) == 307
