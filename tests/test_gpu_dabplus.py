"""DAB+ audio out of ETI on the GPU (dabhip_dabplus_*, eti2aac) against the CPU model of tests/dabplus_model.py: the RS stage bit for bit under
random byte errors, the superframe sync (phases, FCT gap, STL change, fire-code losses, per-stream SubChId sets, any chunking of the pushes),
the whole chain from IQ through Engine.decode, and the CLI."""
import os
import subprocess

import numpy as np
import pytest

import dabplus_model as m
import dabtools_amd as dab
from conftest import fresh_seed

pytestmark = pytest.mark.gpu

FIELDS = ("fct", "s", "fire_ok", "layout_ok", "rfa", "dac_rate", "sbr_flag", "aac_channel_mode", "ps_flag", "mpeg_surround_config", "num_aus",
          "crc_ok", "rs_corrected", "rs_failed")


def _model_stats(recs, losses):
    lay = [r for r in recs if r["layout_ok"]]
    return [len(recs), sum(1 for r in recs if not r["fire_ok"]), sum(r["rs_corrected"] for r in recs), sum(r["rs_failed"] for r in recs),
            sum(r["num_aus"] for r in lay), sum(r["num_aus"] - bin(r["crc_ok"]).count("1") for r in lay), losses]


def _gpu_lane(dp, stream, sub):
    """(records, corrected bytes, good AUs) of the last push of one (stream, sub-channel)."""
    return dp.superframes(stream, sub), dp.data(stream, sub), [bytes(a) for a in dp.aus(stream, sub)]


def _assert_lane_equal(got_recs, got_data, got_aus, want, what):
    assert len(got_recs) == len(want), (what, len(got_recs), len(want))
    for g, w in zip(got_recs, want):
        for f in FIELDS:
            assert int(g[f]) == int(w[f]), (what, f, int(g[f]), int(w[f]))
        assert list(g["au_start"]) == w["au_start"] and list(g["au_len"]) == w["au_len"], what
    want_data = np.concatenate([w["data"] for w in want]) if want else np.zeros(0, np.uint8)
    assert np.array_equal(got_data, want_data), what
    assert got_aus == [a for w in want for a in m.good_aus(w["data"], w)], what


def _protected_superframes(rng, s, nsf):
    out = []
    for _ in range(nsf):
        dac, sbr = [(0, 1), (0, 0), (1, 1), (1, 0)][rng.integers(4)]
        n, start0 = m.AU_LAYOUT[(dac, sbr)]
        hi = min(110 * s - 2, 4095)
        while True:
            cuts = np.sort(rng.choice(np.arange(start0 + 3, hi), n - 1, replace=False))
            b = np.concatenate([[start0], cuts, [110 * s]])
            if np.all(np.diff(b) >= 3):
                break
        aus = [rng.integers(0, 256, int(b[i + 1] - b[i] - 2)).astype(np.uint8).tobytes() for i in range(n)]
        out.append(m.protect(m.pack_superframe(aus, s, dac, sbr, int(rng.integers(2)), int(rng.integers(2)))))
    return out


def _frames(fct0, subs):
    """subs: [(SubChId, [protected superframes])] -> the ETI frames that carry them side by side."""
    nf = 5 * len(subs[0][1])
    frames = []
    for f in range(nf):
        pay = []
        for scid, sfs in subs:
            s = sfs[0].size // 120
            pay.append((scid, sfs[f // 5][24 * s * (f % 5):24 * s * (f % 5 + 1)]))
        frames.append(m.eti_frame((fct0 + f) % 250, pay))
    return frames


def _run(dp, streams, subids, chunk=None):
    """Push streams (lists of frames) whole or in chunks -> {(stream, sub): (records, data, aus)} gathered over the pushes."""
    got = {(b, q): ([], [], []) for b in range(len(streams)) for q in range(len(subids))}
    longest = max(len(f) for f in streams)
    step = chunk or max(longest, 1)
    for a in range(0, longest, step):
        parts = [f[a:a + step] for f in streams]
        dp.push([np.array(p, dtype=np.uint8).reshape(-1, m.ETI_BYTES) if p else np.zeros((0, m.ETI_BYTES), np.uint8) for p in parts])
        for key, (r, d, u) in got.items():
            rr, dd, uu = _gpu_lane(dp, *key)
            r.append(rr)
            d.append(dd)
            u += uu
    return {k: (np.concatenate(r), np.concatenate(d), u) for k, (r, d, u) in got.items()}


def test_rs_stage_equals_the_model_under_random_errors():
    seed = fresh_seed("test_rs_stage_equals_the_model_under_random_errors")
    rng = np.random.default_rng(seed)
    rates = [1, 4, 11, 12, 24, 48, 72]
    ids = [3, 9, 17, 21, 33, 40, 63]
    streams = []
    for b in range(2):
        subs = []
        for scid, s in zip(ids, rates):
            sfs = _protected_superframes(rng, s, 9)
            for sf in sfs:
                for j in range(s):                                      # 0..8 byte errors per codeword, anywhere (fire code, au_start, parity)
                    ne = int(rng.integers(0, 9))
                    k = rng.choice(120, ne, replace=False)
                    sf[j + k * s] ^= rng.integers(1, 256, ne).astype(np.uint8)
            subs.append((scid, sfs))
        streams.append(_frames(int(rng.integers(250)), subs)[int(rng.integers(5)):])
    dp = dab.DabPlus(len(streams), ids)
    assert dp.push(streams) > 0
    fixed = failed = 0
    for b, frames in enumerate(streams):
        for q, scid in enumerate(ids):
            sm = m.SyncModel(scid)
            want = m.stage(sm, frames)
            _assert_lane_equal(*_gpu_lane(dp, b, q), want, (seed, b, scid))
            assert list(dp.stats(b, q)) == _model_stats(want, sm.losses), (seed, b, scid)
            fixed += sum(w["rs_corrected"] for w in want)
            failed += sum(w["rs_failed"] for w in want)
    assert fixed > 0 and failed > 0
    st = dp.stage_ms()
    assert set(st) == {"locate", "sync", "rs", "au", "carry"} and all(v >= 0 for v in st.values())


def test_empty_pushes_and_the_stage_ms_entry():
    """A push without a frame on a fresh object and one that completes no superframe return 0 and leave every query answering (buffers of zero
    records, code words and syndromes); the frames that follow decode as if nothing had happened.  Then dabhip_dabplus_stage_ms's contract: 5
    whatever cap is, min(cap, 5) entries written, null arrays tolerated, a null handle refused."""
    import ctypes as C
    rng = np.random.default_rng(16)
    frames = [_frames(40, [(5, _protected_superframes(rng, 4, 4))]), _frames(90, [(5, _protected_superframes(rng, 4, 4))])[1:]]
    dp = dab.DabPlus(2, [5])
    for parts in ([[], []], [frames[0][:3], []]):
        assert dp.push([np.array(p, dtype=np.uint8).reshape(-1, m.ETI_BYTES) for p in parts]) == 0
        for b in range(2):
            assert dp.superframes(b, 0).size == 0 and dp.data(b, 0).size == 0 and dp.aus(b, 0) == [] and not dp.stats(b, 0).any()
    assert dp.push([np.array(frames[0][3:], dtype=np.uint8), np.array(frames[1], dtype=np.uint8)]) > 0
    for b in range(2):
        sm = m.SyncModel(5)
        want = m.stage(sm, frames[b])
        assert len(want) > 0
        _assert_lane_equal(*_gpu_lane(dp, b, 0), want, b)
        assert list(dp.stats(b, 0)) == _model_stats(want, sm.losses)
    fn, want = dab.lib().dabhip_dabplus_stage_ms, ["locate", "sync", "rs", "au", "carry"]
    for cap in (0, 1, 4, 5, 8):
        names, ms = (C.c_char_p * 8)(), (C.c_float * 8)(*([-7.0] * 8))
        assert fn(dp._h, names, ms, cap) == 5
        k = min(cap, 5)
        assert [n.decode() for n in names[:k]] == want[:k] and all(np.isfinite(v) and v >= 0 for v in ms[:k])
        assert all(n is None for n in names[k:]) and all(v == -7.0 for v in ms[k:])
    names, ms = (C.c_char_p * 5)(), (C.c_float * 5)()
    assert fn(dp._h, None, ms, 5) == 5 and fn(dp._h, names, None, 5) == 5 and fn(dp._h, None, None, 5) == 5 and fn(None, names, ms, 5) == -1
    assert list(dp.stage_ms()) == want
    dp.close()


def test_sync_rule_and_any_chunking_of_the_pushes():
    seed = fresh_seed("test_sync_rule_and_any_chunking_of_the_pushes")
    rng = np.random.default_rng(seed)
    ids = [5, 9, 12]
    streams = []
    for phase in range(5):                                              # streams starting at each of the 5 phases
        streams.append(_frames(int(rng.integers(250)), [(5, _protected_superframes(rng, 4, 10))])[phase:])
    gap = _frames(100, [(5, _protected_superframes(rng, 4, 10))])
    del gap[23]                                                         # an FCT gap
    streams.append(gap)
    streams.append(_frames(7, [(5, _protected_superframes(rng, 4, 5))]) + _frames(32, [(5, _protected_superframes(rng, 8, 5))]))   # STL change
    sfs = _protected_superframes(rng, 4, 10)
    for k in (3, 4, 5):                                                 # K = 3 candidates in a row with a failing raw fire code (RS repairs it)
        sfs[k][0] ^= 0x5A
    streams.append(_frames(240, [(5, sfs)]))                            # the FCT wraps too
    streams.append(_frames(3, [(5, _protected_superframes(rng, 12, 6)), (9, _protected_superframes(rng, 2, 6))])[2:])   # different SubChId sets
    streams.append(_frames(50, [(9, _protected_superframes(rng, 6, 6)), (12, _protected_superframes(rng, 1, 6))]))
    want, losses = {}, {}
    for b, frames in enumerate(streams):
        for q, scid in enumerate(ids):
            sm = m.SyncModel(scid)
            want[b, q] = m.stage(sm, frames)
            losses[b, q] = sm.losses
    assert losses[5, 0] == 1 and losses[6, 0] == 1 and losses[7, 0] == 1
    assert all(len(want[b, 0]) >= 9 - (b > 0) for b in range(5))
    assert [r["fire_ok"] for r in want[7, 0]].count(1) == len(want[7, 0])
    for chunk in (None, 1, 3, 7, 250):
        dp = dab.DabPlus(len(streams), ids)
        got = _run(dp, streams, ids, chunk)
        for key in want:
            _assert_lane_equal(*got[key], want[key], (seed, chunk, key))
            assert list(dp.stats(*key)) == _model_stats(want[key], losses[key]), (seed, chunk, key)
        dp.close()


def _cif_of(cfg, ntf):
    return {dab.synth_fibs(cfg, c).tobytes(): c for c in range(4 * ntf)}


def test_end_to_end_from_iq_through_the_engine_on_device_frames():
    ntf, cfgs = 40, []
    for b in range(4):
        cfg = dab.synth_preset(0, seed=500 + b, cif_count0=(1237 * b) % 5000, skip_samples=9000 * b)
        cfg.dabplus_slots = (1 << cfg.nsub) - 1
        cfg.dabplus_phase = b + 1
        cfgs.append(cfg)
    ids = [cfgs[0].sub[k].id for k in range(cfgs[0].nsub)]
    eng = dab.Engine(0)
    assert eng.decode([dab.synth_generate(c, ntf) for c in cfgs]) > 0
    ptr, total = eng.eti_device_ptr()
    counts = [eng.eti_count(b) for b in range(4)]
    assert sum(counts) == total and min(counts) >= 80
    dp = dab.DabPlus(4, ids)
    assert dp.push((ptr, counts)) > 0
    for b, cfg in enumerate(cfgs):
        frames = eng.eti(b)
        cif_index = _cif_of(cfg, ntf)
        cifs = [cif_index[f[12 + 4 * (f[5] & 0x7f):][:96].tobytes()] for f in frames]
        fct_pos = {int(f[4]): i for i, f in enumerate(frames)}
        for q in range(len(ids)):
            recs = dp.superframes(b, q)
            aus = [bytes(a) for a in dp.aus(b, q)]
            # every superframe whose 5 CIFs are all in the capture, from the first one on
            complete = [n for n in range(-4, 4 * ntf) if all(cfg.dabplus_phase + 5 * n + k in cifs for k in range(5))]
            assert [(cifs[fct_pos[int(r["fct"])]] - cfg.dabplus_phase) // 5 for r in recs] == complete, (b, q)
            want = []
            for n in complete:
                u = dab.synth_dabplus_superframe(cfg, n, q)
                want += m.good_aus(u, m.parse(u))
            assert aus == want, (b, q)
            assert all(r["fire_ok"] and r["layout_ok"] and r["rs_corrected"] == 0 and r["rs_failed"] == 0 and r["crc_ok"] == (1 << r["num_aus"]) - 1
                       for r in recs)


def test_noisy_capture_gpu_equals_the_model_on_the_same_eti():
    ntf, cfgs = 40, []
    for b in range(2):
        cfg = dab.synth_preset(0, seed=700 + b, cif_count0=311 * b, snr_db=7.0)
        cfg.dabplus_slots = (1 << cfg.nsub) - 1
        cfg.dabplus_phase = 2 * b
        cfgs.append(cfg)
    ids = [cfgs[0].sub[k].id for k in range(cfgs[0].nsub)]
    eng = dab.Engine(0)
    assert eng.decode([dab.synth_generate(c, ntf) for c in cfgs]) > 0
    streams = [list(eng.eti(b)) for b in range(2)]
    dp = dab.DabPlus(2, ids)
    dp.push([np.array(f) for f in streams])
    fixed = 0
    for b in range(2):
        for q, scid in enumerate(ids):
            sm = m.SyncModel(scid)
            want = m.stage(sm, streams[b])
            _assert_lane_equal(*_gpu_lane(dp, b, q), want, (b, scid))
            assert list(dp.stats(b, q)) == _model_stats(want, sm.losses)
            fixed += sum(w["rs_corrected"] for w in want)
    assert fixed > 0


def test_cli_dab2eti_pipe_eti2aac(tmp_path):
    here = os.path.dirname(dab.LIB_PATH)
    ntf = 30
    cfg = dab.synth_preset(0, seed=91, cif_count0=4990)
    cfg.dabplus_slots = (1 << cfg.nsub) - 1
    cfg.dabplus_phase = 3
    cap = tmp_path / "cap.cu8"
    dab.synth_generate(cfg, ntf).tofile(cap)
    eti = subprocess.run([os.path.join(here, "dab2eti-hip"), str(cap)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout
    frames = list(np.frombuffer(eti, np.uint8).reshape(-1, m.ETI_BYTES))
    cif_index = _cif_of(cfg, ntf)
    for slot in (0, 5, 10):
        scid = cfg.sub[slot].id
        recs = m.stage(m.SyncModel(scid), frames)
        assert len(recs) >= 8
        for r in recs:                                                 # the model's AUs are the synth's
            f = frames[[int(x[4]) for x in frames].index(r["fct"])]
            n = (cif_index[f[12 + 4 * (f[5] & 0x7f):][:96].tobytes()] - cfg.dabplus_phase) // 5
            u = dab.synth_dabplus_superframe(cfg, n, slot)
            assert m.good_aus(r["data"], r) == m.good_aus(u, m.parse(u))
        cmd = "set -o pipefail; '%s' '%s' | '%s' %s%d" % (os.path.join(here, "dab2eti-hip"), cap, os.path.join(here, "eti2aac"), "%s", scid)
        adts = subprocess.run(["bash", "-c", cmd % ""], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert adts.returncode == 0, adts.stderr
        assert adts.stdout == m.adts_stream(recs)
        assert b"eti2aac: %d frames" % len(frames) in adts.stderr and b"%d superframes" % len(recs) in adts.stderr
        raw = subprocess.run(["bash", "-c", cmd % "--raw "], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert raw.returncode == 0 and raw.stdout == b"".join(a for r in recs for a in m.good_aus(r["data"], r))
