"""The MPEG-2 TS kernels (k_ts.hip through Ts.push) against the model of ts_model.py, bit for bit: records, the packets' 188 bytes and the
counters.  ETI frames are built by hand from the model and the crafted classes of ts_cases.py: Reed-Solomon words at the decoder's edges, byte
streams at the edges of the sync rule and of the 64-slot ballot, every kind of break; sub-channels from 24 bytes per frame (the look-ahead
spans 102 frames) to the largest the frame holds, side by side in one handle; 63 to 129 slots per lane, 5 lanes (one more than a sync
workgroup's waves) and 1023 to 2049 lanes; every way frames arrive and any cutting into pushes, pushes of 0 and 1 frame included; and
modulated captures through the decoder, the stage and eti2ts against the modulator's own words."""
import os
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import ts_cases as cs
import ts_model as m

pytestmark = pytest.mark.gpu


def _gpu_lane(ts, b, q):
    recs = ts.records(b, q)
    return [(int(r["pos"]), int(r["pid"]), int(r["continuity"]), int(r["flags"]), int(r["corrected"])) for r in recs], ts.data(b, q)


def _cuts(nframes, chunk, rng):
    """Frame counts of the pushes: fixed, or random with pushes of 0 and 1 frame among them."""
    if chunk is None:
        return [nframes]
    if chunk != "random":
        return [min(chunk, nframes - a) for a in range(0, nframes, chunk)] or [0]
    out, left = [0, 1], nframes - 1
    while left > 0:
        n = int(rng.choice([0, 1, 2, 5, 17, 60, 103, 200]))
        out.append(min(n, left))
        left -= out[-1]
    return out if nframes > 0 else [0]


def _run(ts, streams, nsub, chunk=None, how="host", seed=0, lanes=None):
    """Push the streams in cuts (the same cut positions for every stream) -> {(stream, sub): (records, bytes)} of the lanes asked for"""
    rng = np.random.default_rng(seed)
    longest = max(len(f) for f in streams)
    keys = lanes if lanes is not None else [(b, q) for b in range(len(streams)) for q in range(nsub)]
    got = {k: ([], []) for k in keys}
    total, at, seen = 0, 0, 0
    for n in _cuts(longest, chunk, rng):
        parts = [f[at:at + n] for f in streams]
        at += n
        counts = [len(p) for p in parts]
        flat = np.concatenate([np.asarray(f, np.uint8).reshape(-1) for p in parts for f in p]) if sum(counts) else np.zeros(0, np.uint8)
        buf = None
        if how == "host":
            total += ts.push(flat, counts)
        else:
            off = 1 if how == "device+1" else 0
            buf = dab.DeviceBuffer(flat.size + 16)
            assert buf.ptr % 16 == 0
            buf.upload(np.concatenate([np.zeros(off, np.uint8), flat]))
            total += ts.push((buf.ptr + off, counts))
        for key, (r, d) in got.items():
            rr, dd = _gpu_lane(ts, *key)
            r += rr
            d.append(dd)
            seen += len(rr)
        if buf is not None:
            buf.free()
    if lanes is None:
        assert total == seen
    return {k: (r, np.concatenate(d)) for k, (r, d) in got.items()}, total


def _expect(streams, ids):
    """The model over whole streams -> ({(stream, sub): (records, bytes)}, {(stream, sub): statistics})"""
    want, stats = {}, {}
    for b, frames in enumerate(streams):
        for q, scid in enumerate(ids):
            lane = m.Lane(scid)
            want[b, q] = lane.push(frames)
            stats[b, q] = lane.stat_list()
    return want, stats


def _assert_equal(ts, got, want, stats, ctx):
    for key, (grecs, gdata) in got.items():
        recs, data = want[key]
        assert len(grecs) == len(recs), (ctx, key, len(grecs), len(recs))
        for i, (a, b) in enumerate(zip(grecs, recs)):
            assert a == tuple(b), (ctx, key, i, a, b)
        assert gdata.shape == data.shape and (gdata == data).all(), (ctx, key)
        assert list(ts.stats(*key)) == stats[key], (ctx, key, list(ts.stats(*key)), stats[key])


def _check(streams, ids, plans, ctx, expect=None):
    want, stats = expect or _expect(streams, ids)
    for chunk, how in plans:
        ts = dab.Ts(len(streams), ids)
        got, _ = _run(ts, streams, len(ids), chunk, how, seed=len(streams))
        _assert_equal(ts, got, want, stats, (ctx, chunk, how))
        ts.close()
    return want, stats


def test_rs_classes_through_the_stage():
    """Every crafted word's error pattern on a code word of a real stream, a clean word between any two: a corrected word comes out as sent, a
    word left as received or miscorrected shows in the bytes, the flags and the counters exactly as the model has it."""
    stream, npat = cs.rs_stream(np.random.default_rng(41))
    assert npat > 350
    frames = cs.frames_of_bytes(11, [(6, 204, stream)])
    want, stats = _check([frames], [6], [(None, "host"), (7, "device")], "rs")
    st = dict(zip(m.STATS, stats[0, 0]))
    # by construction: every word of classes e8, e1, parity and miscorrect is corrected, every word of classes shortened and beyond fails
    assert st["rs_failed_words"] >= 10 + 290 and st["rs_corrected_bytes"] >= 12 * 8 + 5 + 13 + 8 * 8 and st["sync_losses"] == 0, st
    assert st["packets"] >= 2 * npat and st["from_missed_slots"] > 0 and st["bad_sync_packets"] > 0, st


SIZES = (3, 24, 26, 51, 204, 205, 306, m.STL_MAX)
_SIZE_STREAMS = None


def _size_streams():
    """A stream per STL of SIZES, each from a random phase behind some junk, with byte errors, a few words beyond correction and knocked-out sync
    bytes (never three in a row); the model's answer, computed once."""
    global _SIZE_STREAMS
    if _SIZE_STREAMS is None:
        rng = np.random.default_rng(306)
        streams = []
        for stl in SIZES:
            per = 8 * stl
            nframes = max(30, -(-4200 // per))                 # at STL 3: 175 frames of 24 bytes, the look-ahead alone is 102 of them
            nj, phase = int(rng.integers(0, 300)), int(rng.integers(0, m.SLOT))
            length = nframes * per - nj
            first, count = m.words_needed(phase, length)
            errors = {}
            for n in rng.choice(np.arange(first + 12, first + count), min(count // 8, 40), replace=False):
                e = np.zeros(m.N, np.uint8)
                ne = int(rng.choice([1, 2, 8, 9, 12]))
                e[rng.choice(m.N, ne, replace=False)] = rng.integers(1, 256, ne)
                errors[int(n)] = e
            s = np.concatenate([cs.junk(rng, nj), cs.clean_stream(rng, length, phase, errors)[0]])
            streams.append(cs.frames_of_bytes(stl, [(5, stl, s)], ficf=0 if stl == m.STL_MAX else 1))
            assert len(streams[-1]) == nframes
        _SIZE_STREAMS = (streams, _expect(streams, [5]))
    return _SIZE_STREAMS


@pytest.mark.parametrize("chunk,how", [(None, "host"), (None, "device"), (1, "device"), ("random", "host"), ("random", "device+1")])
def test_stream_sizes_side_by_side(chunk, how):
    """A lane at each STL of SIZES in one handle: below one slot per frame, just above, exactly two and eight, exactly the look-ahead, the
    largest the locate rule accepts with NST = 1.  In pushes of one frame a run's five bytes and a word's 204 lie across the carry and up to
    102 new frames; unaligned device frames are read byte by byte."""
    streams, (want, stats) = _size_streams()
    _check(streams, [5], [(chunk, how)], "sizes", expect=(want, stats))
    for b, stl in enumerate(SIZES):
        st = dict(zip(m.STATS, stats[b, 0]))
        assert st["packets"] >= 6 and st["sync_losses"] == 0, (stl, st)
    total = np.sum([stats[k] for k in stats], axis=0)
    assert total[4] > 50 and total[5] > 5 and total[1] > 0, total


def test_sync_classes_through_the_stage():
    sync = cs.sync_streams()
    labels = sorted(sync)
    streams = [cs.sync_frames(sync[k][0], 5 * i) for i, k in enumerate(labels)]
    want, stats = _check(streams, [cs.SYNC_ID], [(None, "host"), (3, "host"), (1, "device"), ("random", "device+1")], "sync")
    for i, k in enumerate(labels):
        st = dict(zip(m.STATS, stats[i, 0]))
        for name, v in sync[k][1].items():
            assert st[name] == v, (k, name, st)


def test_three_misses_at_the_ballot_border_and_at_the_last_slots_with_look_ahead():
    """One push from scratch: the lane syncs at its phase, so slot i of the stream is slot i of the sync kernel's first chunk of 64.  Three
    misses on slots 61-62-63 (the loss is the chunk's last slot), 62-63-64 (two misses carried into the next chunk), 63-64-65 (one carried);
    two misses at the border, which lose nothing; and three on the last slots that have their look-ahead."""
    rng = np.random.default_rng(64)
    per, nframes, phase = 8 * cs.SYNC_STL, 60, 40
    length = nframes * per
    last = (length - phase - m.LOOK) // m.SLOT              # the last slot with its look-ahead
    assert last > 70
    cases = {"61-63": (61, 62, 63), "62-64": (62, 63, 64), "63-65": (63, 64, 65), "two at the border": (63, 64), "the last three": (last - 2, last - 1, last),
             "the last two": (last - 1, last)}
    streams, labels = [], sorted(cases)
    for k in labels:
        s, _, _ = cs.clean_stream(rng, length, phase)
        for n in cases[k]:
            s[phase + m.SLOT * n] ^= 0x5A
        streams.append(cs.sync_frames(s))
    want, stats = _check(streams, [cs.SYNC_ID], [(None, "host"), (None, "device+1"), ("random", "host")], "border")
    for i, k in enumerate(labels):
        st = dict(zip(m.STATS, stats[i, 0]))
        three = len(cases[k]) == 3
        assert st["sync_losses"] == int(three) and st["from_missed_slots"] == 2 and st["packets"] == last + 1 - int(three), (k, st)
        # a loss skips one byte and then the 203 up to the next slot, where the next run of five starts (after the last slot with its look-ahead
        # there are still eleven slots on hand, so that run is decided in the same push)
        assert st["bytes_skipped"] == phase + (m.SLOT if three else 0), (k, st)


@pytest.mark.parametrize("chunk,how", [(None, "host"), ("random", "device")])
def test_slots_per_lane_and_one_lane_more_than_a_workgroup_has_waves(chunk, how):
    """Five lanes (a sync workgroup holds four waves) of 63, 64, 65, 128 and 129 decidable slots: the ballot's chunk exactly full, one short, one
    over, and the same at two chunks."""
    rng = np.random.default_rng(129)
    stl, streams = 51, []
    for nslots in (63, 64, 65, 128, 129):
        # bytes on hand: the last slot's look-ahead ends with the last frame, or up to 203 bytes before it
        nframes = -(-(m.SLOT * (nslots - 1) + m.LOOK) // (8 * stl))
        phase = nframes * 8 * stl - (m.SLOT * (nslots - 1) + m.LOOK)
        assert 0 <= phase < 8 * stl
        s = np.concatenate([cs.junk(rng, phase), cs.clean_stream(rng, nframes * 8 * stl - phase, 0)[0]])      # the first slot starts behind the junk
        s[rng.choice(s.size, s.size // 700, replace=False)] ^= 0x21
        streams.append(cs.frames_of_bytes(1, [(9, stl, s)]))
    want, stats = _check(streams, [9], [(chunk, how)], "slots")
    assert [stats[b, 0][0] for b in range(5)] == [63, 64, 65, 128, 129]


_SHORT = None


def _short_streams():
    """Seven short streams (two frames at the largest STL: 47 or 48 packets) and the model's answers."""
    global _SHORT
    if _SHORT is None:
        rng = np.random.default_rng(2049)
        streams = []
        for i in range(7):
            s, _, _ = cs.clean_stream(rng, 2 * 8 * m.STL_MAX, 29 * i)
            s[rng.choice(s.size, 25, replace=False)] ^= 0x80
            streams.append(cs.frames_of_bytes(i, [(33, m.STL_MAX, s)], ficf=0))
        _SHORT = (streams, _expect(streams, [33]))
    return _SHORT


@pytest.mark.parametrize("nlanes", (1023, 1024, 1025, 2049))
def test_many_lanes_on_short_streams(nlanes):
    """Around the scan kernel's 1024 threads and past twice that: lane b carries short stream b mod 7, every 13th lane and the last ones are read
    back whole, and the push's total is the sum over all."""
    short, (want, stats) = _short_streams()
    streams = [short[b % 7] for b in range(nlanes)]
    lanes = sorted(set(list(range(0, nlanes, 13)) + [nlanes - 2, nlanes - 1]))
    ts = dab.Ts(nlanes, [33])
    got, total = _run(ts, streams, 1, None, "host", lanes=[(b, 0) for b in lanes])
    assert total == sum(len(want[b % 7, 0][0]) for b in range(nlanes))
    _assert_equal(ts, got, {(b, 0): want[b % 7, 0] for b in lanes}, {(b, 0): stats[b % 7, 0] for b in lanes}, nlanes)
    ts.close()


def test_breaks_an_id_listed_twice_and_bad_stls():
    """Every kind of break behind units of the same push (absent, STL 0, a payload past byte 6144, another STL and back), an id listed twice whose
    first entry counts, a break with no sync to lose; next to an unbroken lane of another id in the same frames' handle."""
    frames, losses = cs.broken_frames()
    want, stats = _check([frames, frames[:60]], [cs.SYNC_ID, 8], [(None, "host"), (50, "device"), (1, "host"), ("random", "device+1")], "breaks")
    st = dict(zip(m.STATS, stats[0, 0]))
    assert st["sync_losses"] == losses and st["packets"] > 100 and st["rs_failed_words"] == 0, st
    assert stats[0, 1][0] == 0 and stats[0, 1][3] > 0          # id 8 shows in three frames only, far apart: bytes skipped, no packets


def test_stage_times_empty_pushes_and_refusals():
    ts = dab.Ts(2, [1, 2])
    assert ts.push(np.zeros(0, np.uint8), [0, 0]) == 0
    assert tuple(ts.stage_ms()) == dab.TS_STAGES and all(v >= 0 for v in ts.stage_ms().values())
    assert ts.records(1, 1).size == 0 and ts.data(0, 0).shape == (0, 188) and list(ts.stats(1, 0)) == [0] * 8
    stream, _, _ = cs.clean_stream(np.random.default_rng(1), 40 * 408, 3)
    frames = cs.frames_of_bytes(0, [(2, 51, stream)])
    n = ts.push(np.array(frames[:25]), [25, 0]) + ts.push(np.zeros(0, np.uint8), [0, 0]) + ts.push(np.array(frames[25:]), [15, 0])
    assert ts.push(np.zeros(0, np.uint8), [0, 0]) == 0 and ts.records(0, 1).size == 0      # an empty push: no packets, the state stays
    lane = m.Lane(2)
    assert n == len(lane.push(frames)[0]) > 60 and list(ts.stats(0, 1)) == lane.stat_list()
    ms = ts.stage_ms()
    assert tuple(ms) == dab.TS_STAGES and all(v >= 0 for v in ms.values())
    with pytest.raises(dab.DabhipError):
        ts.records(2, 0)
    with pytest.raises(dab.DabhipError):
        ts.stats(0, 2)
    with pytest.raises(dab.DabhipError):
        ts.push(np.zeros(0, np.uint8), [-1, 0])
    ts.close()
    with pytest.raises(dab.DabhipError):
        dab.Ts(1, [64])
    with pytest.raises(dab.DabhipError):
        dab.Ts(0, [1])
    with pytest.raises(dab.DabhipError):
        dab.Ts(1, list(range(64)) + [1])


# ---- end to end: modulated captures through the decoder and the stage ----------------------------------------------------------------------------
def _cifs_of(cfg, frames, ntf):
    index = {dab.synth_fibs(cfg, c).tobytes(): c for c in range(4 * ntf)}
    cifs = [index[f[12 + 4 * (f[5] & 0x7f):][:96].tobytes()] for f in frames]
    assert cifs == list(range(cifs[0], cifs[0] + len(cifs)))
    return cifs


def _truth(cfg, slot, cifs):
    """The packets a lane must give for the frames of the consecutive logical CIFs `cifs` of a ts_slots slot: (positions, [n][188] bytes) from
    the modulator's own words -- every slot that starts in the frames and has its 2448 bytes in them."""
    per = dab.synth_payload(cfg, 0, slot).size
    x0, x1 = cifs[0] * per, (cifs[-1] + 1) * per
    n0 = -(-(x0 - cfg.ts_phase) // m.SLOT)
    n1 = (x1 - m.LOOK - cfg.ts_phase) // m.SLOT
    pos = [m.SLOT * n + cfg.ts_phase - x0 for n in range(n0, n1 + 1)]
    data = np.stack([dab.synth_ts_word(cfg, slot, n)[:m.K] for n in range(n0, n1 + 1)]) if n1 >= n0 else np.zeros((0, m.K), np.uint8)
    return pos, data


def _ts_cfg(seed, phase, **kw):
    cfg = dab.synth_preset(0, seed=seed, **kw)
    cfg.ts_slots = (1 << cfg.nsub) - 1
    cfg.ts_phase = phase
    return cfg


def test_end_to_end_from_iq_through_the_engine_on_device_frames():
    ntf = 40
    cfgs = [_ts_cfg(700 + b, 19 + 150 * b, cif_count0=(2237 * b) % 5000, skip_samples=7000 * b) for b in range(2)]
    nsub = cfgs[0].nsub
    ids = [cfgs[0].sub[k].id for k in range(nsub)]
    eng = dab.Engine(0)
    assert eng.decode([dab.synth_generate(c, ntf) for c in cfgs]) > 0
    ptr, total = eng.eti_device_ptr()
    counts = [eng.eti_count(b) for b in range(2)]
    assert sum(counts) == total and min(counts) >= 80
    ts = dab.Ts(2, ids)
    assert ts.push((ptr, counts)) > 0
    packets = 0
    for b, cfg in enumerate(cfgs):
        cifs = _cifs_of(cfg, eng.eti(b), ntf)
        for q in range(nsub):
            pos, data = _truth(cfg, q, cifs)
            recs, got = ts.records(b, q), ts.data(b, q)
            st = dict(zip(dab.TS_STATS, ts.stats(b, q)))
            assert recs["pos"].tolist() == pos and (got == data).all(), (b, q, st)
            assert st["packets"] == len(pos) and (not pos or st["bytes_skipped"] == pos[0]) and sum(ts.stats(b, q)[[1, 2, 4, 5, 6]]) == 0, (b, q, st)
            assert (recs["flags"] & (0xFF ^ dab.TS_PUSI) == 0).all() and (recs["pid"] == ((data[:, 1].astype(int) & 0x1F) << 8 | data[:, 2])).all()
            assert st["null_packets"] == int((recs["pid"] == m.NULL_PID).sum())
            packets += len(pos)
    assert packets > 2000                                  # (the slowest slots have fewer bytes in these frames than one word's look-ahead)
    ts.close()


def test_cli_dab2eti_pipe_eti2ts(tmp_path):
    here = os.path.dirname(dab.LIB_PATH)
    ntf = 40
    cfg = _ts_cfg(93, 77, cif_count0=4990)
    cap = tmp_path / "cap.cu8"
    dab.synth_generate(cfg, ntf).tofile(cap)
    eti = subprocess.run([os.path.join(here, "dab2eti-hip"), str(cap)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout
    frames = np.frombuffer(eti, np.uint8).reshape(-1, m.ETI_BYTES)
    cifs = _cifs_of(cfg, list(frames), ntf)
    slot = 5
    scid = cfg.sub[slot].id
    pos, data = _truth(cfg, slot, cifs)
    assert len(pos) > 50 and len(frames) >= 80
    cmd = "set -o pipefail; '%s' '%s' | '%s' %d%s" % (os.path.join(here, "dab2eti-hip"), cap, os.path.join(here, "eti2ts"), scid, "%s")
    for flag in ("", " --drop-failed"):
        run = subprocess.run(["bash", "-c", cmd % flag], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert run.returncode == 0, run.stderr
        assert run.stdout == data.tobytes(), flag
        assert b"eti2ts: %d frames" % len(frames) in run.stderr and b" %d packets (%d written)" % (len(pos), len(pos)) in run.stderr, run.stderr
    # the same frames with bytes of the sub-channel broken, so that some words fail: written as received with the transport_error_indicator
    # set, or left out
    broken = frames.copy()
    rng = np.random.default_rng(8)
    off = 12 + 4 * int(broken[0, 5] & 0x7f) + 96 + sum(dab.synth_payload(cfg, 0, k).size for k in range(slot))
    per = dab.synth_payload(cfg, 0, slot).size
    assert (broken[3, off:off + per] == dab.synth_payload(cfg, cifs[3], slot)).all()
    for f in (30, 31, 55):
        at = rng.choice(per, per // 6, replace=False)
        broken[f, off + at] ^= rng.integers(1, 256, at.size).astype(np.uint8)
    recs, want = m.Lane(scid).push(list(broken))
    failed = np.array([bool(r[3] & m.RS_FAILED) for r in recs])
    assert 3 < failed.sum() < len(recs) // 2
    marked = want.copy()
    marked[failed, 1] |= 0x80
    path = tmp_path / "broken.eti"
    broken.tofile(path)
    for flag, expect in (("", marked), ("--drop-failed", want[~failed])):
        with open(path, "rb") as src:
            run = subprocess.run([os.path.join(here, "eti2ts"), str(scid)] + ([flag] if flag else []), stdin=src, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert run.returncode == 0, run.stderr
        assert run.stdout == expect.tobytes(), flag
        assert b"%d RS failed code words" % failed.sum() in run.stderr and b"(%d written)" % len(expect) in run.stderr, run.stderr
