"""The EDI kernels (k_edi.hip through Edi.push) against the model of edi_model.py, bit for bit: the packets' bytes, their records and the
counters; and edi_model.unpack of the GPU's bytes against the frames.  ETI frames are built by hand at the borders of the rules
(edi_cases.py), not for size: NST 0..7, 64, STL 0, FICF 0, every TAG padding, the packet sizes around each chunk-count border, z = 0 and c - 1,
f s = B and not, the three skip reasons, a main stream ending at byte 6140; streams of 0 to 65 frames, 5 unequal streams, 257 and 1025 streams;
every way frames arrive and any cutting into pushes; reset; 5001 frames through FCTH 19 -> 0; and modulated captures through the decoder, the
stage and eti2edi."""
import os
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import edi_cases as cs
import edi_model as m

pytestmark = pytest.mark.gpu

MODES = [(0, 0, 1400), (1, 0, 64), (1, 0, 1472), (2, 0, 1472), (2, 2, 1400), (2, 5, 64)]


def _cuts(nframes, chunk, rng):
    if chunk is None:
        return [nframes]
    if chunk != "random":
        return [min(chunk, nframes - a) for a in range(0, nframes, chunk)] or [0]
    out, left = [0, 1], nframes - 1
    while left > 0:
        n = int(rng.choice([0, 1, 2, 5, 17, 60]))
        out.append(min(n, left))
        left -= out[-1]
    return out if nframes > 0 else [0]


def _recs(edi, b, base):
    return [(base + int(r["offset"]), int(r["length"]), int(r["frame"]), int(r["seq"]), int(r["findex"]), int(r["fcount"])) for r in edi.records(b)]


def _run(edi, streams, chunk=None, how="host", seed=0, watch=None):
    """Push the streams in cuts (the same cut positions for every stream) -> {stream: (bytes, records)} of the streams watched, and the packets"""
    rng = np.random.default_rng(seed)
    longest = max(len(f) for f in streams)
    watch = list(range(len(streams))) if watch is None else watch
    data, recs = {b: [] for b in watch}, {b: [] for b in watch}
    total, at = 0, 0
    for n in _cuts(longest, chunk, rng):
        parts = [f[at:at + n] for f in streams]
        at += n
        counts = [len(p) for p in parts]
        flat = np.concatenate([np.asarray(f, np.uint8).reshape(-1) for p in parts for f in p]) if sum(counts) else np.zeros(0, np.uint8)
        buf = None
        if how == "host":
            total += edi.push(flat, counts)
        else:
            off = 1 if how == "device+1" else 0
            buf = dab.DeviceBuffer(flat.size + 16)
            assert buf.ptr % 16 == 0
            buf.upload(np.concatenate([np.zeros(off, np.uint8), flat]))
            total += edi.push((buf.ptr + off, counts))
        for b in watch:
            recs[b] += _recs(edi, b, sum(x.size for x in data[b]))
            data[b].append(edi.data(b))
        if buf is not None:
            buf.free()
    return {b: (np.concatenate(data[b]), recs[b]) for b in watch}, total


def _expect(streams, mode, recover, max_frag, seq0=0):
    want, stats = {}, {}
    for b, frames in enumerate(streams):
        st = m.Stream(mode, recover, max_frag, seq0)
        want[b] = st.push(frames)
        stats[b] = st.stat_list()
    return want, stats


def _assert_equal(edi, got, want, stats, ctx):
    for b, (gdata, grecs) in got.items():
        data, recs = want[b]
        assert len(grecs) == len(recs), (ctx, b, len(grecs), len(recs))
        for i, (x, y) in enumerate(zip(grecs, recs)):
            assert x == y, (ctx, b, i, x, y)
        assert gdata.size == data.size, (ctx, b, gdata.size, data.size)
        bad = np.nonzero(gdata != data)[0]
        assert bad.size == 0, (ctx, b, bad[:8], [r for r in recs if r[0] <= bad[0] < r[0] + r[1]])
        assert list(edi.stats(b)) == stats[b], (ctx, b, list(edi.stats(b)), stats[b])


def _check(streams, mode, recover, max_frag, plans, ctx, seq0=0, expect=None):
    want, stats = expect or _expect(streams, mode, recover, max_frag, seq0)
    for chunk, how in plans:
        edi = dab.Edi(len(streams), mode, recover, max_frag, seq0)
        got, total = _run(edi, streams, chunk, how, seed=len(streams))
        assert total == sum(len(want[b][1]) for b in want)
        _assert_equal(edi, got, want, stats, (ctx, chunk, how))
        edi.close()
    return want, stats


def _unpacks_to(data, mode, frames, seq0=0):
    fields, _ = m.unpack(data, mode)
    kept = [f for f in frames if m.accepted(f) is not None]
    assert len(fields) == len(kept)
    for i, (x, f) in enumerate(zip(fields, kept)):
        assert m.same_fields(x, f) and x["seq"] == (seq0 + i) & 0xFFFF, i
    return fields


_BORDER = {}


def _border(mode, recover, max_frag):
    key = (mode, recover, max_frag)
    if key not in _BORDER:
        frames = cs.border_frames()
        if mode == 2:
            rng = np.random.default_rng(9)
            frames += [cs.frame_of_l(rng, l, 100 + i) for i, l in enumerate(cs.size_borders(recover, max_frag).values())]
        _BORDER[key] = (frames, _expect([frames], mode, recover, max_frag, 65534))
    return _BORDER[key]


@pytest.mark.parametrize("mode,recover,max_frag", MODES)
def test_border_frames_every_way_they_arrive(mode, recover, max_frag):
    """One stream of the crafted frames, seq0 = 65534: as one host push, device pushes of 7, and random cuts of unaligned device frames with
    pushes of 0 and 1 frame.  Then the receiver's view of the GPU's bytes against the frames."""
    frames, expect = _border(mode, recover, max_frag)
    _check([frames], mode, recover, max_frag, [(None, "host"), (7, "device"), ("random", "device+1")], "border", 65534, expect)
    edi = dab.Edi(1, mode, recover, max_frag, 65534)
    edi.push(np.concatenate(frames))
    _unpacks_to(edi.data(0), mode, frames, 65534)
    edi.close()


@pytest.mark.parametrize("how", ["host", "device", "device+1"])
def test_unaligned_and_aligned_device_frames_in_one_push(how):
    frames, expect = _border(2, 2, 1400)
    _check([frames], 2, 2, 1400, [(None, how), (7, how), ("random", how)], how, 65534, expect)


def _wrapping(rng, n, first=240):
    """n small frames whose FCT runs 240, 241, .. 249, 0, .., every 7th skipped"""
    return [cs.small_frame(rng, (first + i) % 250, skipped=i % 7 == 3) for i in range(n)]


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65])
def test_stream_lengths_around_the_scan_step(n):
    """The scan kernel takes 64 frames per step: a stream just below, at and above it, with FCT wraps and skipped frames in it."""
    rng = np.random.default_rng(n)
    frames = _wrapping(rng, n)
    for mode, recover, max_frag in ((0, 0, 1400), (2, 1, 64)):
        if n == 0:
            edi = dab.Edi(1, mode, recover, max_frag)
            assert edi.push(np.zeros(0, np.uint8), [0]) == 0 and edi.data(0).size == 0 and edi.records(0).size == 0 and list(edi.stats(0)) == [0] * 6
            edi.close()
        else:
            _check([frames], mode, recover, max_frag, [(None, "host"), ("random", "device")], n)


def test_five_streams_of_unequal_length():
    """One more stream than a scan workgroup has waves; the FCT of each starts elsewhere, so the wraps fall at different frames."""
    rng = np.random.default_rng(5)
    streams = [_wrapping(rng, n, first) for n, first in ((70, 249), (1, 0), (130, 200), (64, 186), (33, 10))]
    streams[2][100:103] = cs.border_frames()[9:12]
    for mode, recover, max_frag in ((1, 0, 64), (2, 5, 64)):
        _check(streams, mode, recover, max_frag, [(None, "host"), (7, "device"), ("random", "device+1")], "five")


@pytest.mark.parametrize("nstreams", [257, 1025])
def test_many_streams_of_three_frames(nstreams):
    """Around the bases kernel's 1024 threads: stream b carries one of 7 short streams; every 13th stream and the last ones are read back whole."""
    rng = np.random.default_rng(1025)
    short = [[cs.frame(rng, (248 + i) % 250, [int(v) for v in rng.integers(0, 12, b % 4)], ficf=b % 2) for i in range(3)] for b in range(7)]
    want, stats = _expect(short, 2, 2, 255)
    streams = [short[b % 7] for b in range(nstreams)]
    watch = sorted(set(list(range(0, nstreams, 13)) + [nstreams - 2, nstreams - 1]))
    edi = dab.Edi(nstreams, 2, 2, 255)
    got, total = _run(edi, streams, None, "host", watch=watch)
    assert total == sum(len(want[b % 7][1]) for b in range(nstreams))
    _assert_equal(edi, got, {b: want[b % 7] for b in watch}, {b: stats[b % 7] for b in watch}, nstreams)
    edi.close()


def test_reset_of_one_stream_among_others():
    rng = np.random.default_rng(20)
    streams = [_wrapping(rng, 12, 245 + b) for b in range(3)]
    edi = dab.Edi(3, 2, 1, 255, 9)
    models = [m.Stream(2, 1, 255, 9) for _ in range(3)]
    for step in range(3):
        got, _ = _run(edi, streams)
        want = {b: models[b].push(streams[b]) for b in range(3)}
        _assert_equal(edi, got, want, {b: models[b].stat_list() for b in range(3)}, ("reset", step))
        edi.reset(1)
        models[1].reset()
    with pytest.raises(dab.DabhipError):
        edi.reset(3)
    edi.close()


def test_a_long_stream_through_fcth_19_to_0():
    """5001 frames in mode 0, FCT 0..249 twenty times over: the frame behind the 20th wrap has FCTH 0 again."""
    rng = np.random.default_rng(5001)
    frames = [cs.small_frame(rng, i % 250) for i in range(5001)]
    want, stats = _check([frames], 0, 0, 1400, [(None, "host"), (1000, "device")], "long")
    fields, _ = m.unpack(want[0][0], 0)
    assert [fields[i]["fcth"] for i in (0, 249, 250, 4749, 4750, 4999, 5000)] == [0, 0, 1, 18, 19, 19, 0]
    assert fields[-1]["seq"] == 5000 and stats[0][0] == 5001


def test_stage_times_empty_pushes_and_refusals():
    edi = dab.Edi(2, 2, 2, 1400)
    assert edi.push(np.zeros(0, np.uint8), [0, 0]) == 0
    assert tuple(edi.stage_ms()) == dab.EDI_STAGES and all(v >= 0 for v in edi.stage_ms().values())
    assert edi.records(1).size == 0 and edi.data(0).size == 0 and list(edi.stats(1)) == [0] * 6
    frames = cs.border_frames()
    n = edi.push(np.array(frames[:9]), [9, 0]) + edi.push(np.zeros(0, np.uint8), [0, 0])
    assert edi.records(0).size == 0 and edi.data(0).size == 0          # an empty push: no packets, the state stays
    n += edi.push(np.array(frames[9:]), [len(frames) - 9, 0])
    st = m.Stream(2, 2, 1400)
    assert n == len(st.push(frames)[1]) > 50 and list(edi.stats(0)) == st.stat_list() and list(edi.stats(1)) == [0] * 6
    ms = edi.stage_ms()
    assert tuple(ms) == dab.EDI_STAGES and all(v >= 0 for v in ms.values())
    for call in (lambda: edi.records(2), lambda: edi.data(-1), lambda: edi.stats(2), lambda: edi.push(np.zeros(0, np.uint8), [-1, 0]),
                 lambda: edi.push(np.zeros(0, np.uint8), [1 << 18, 0])):
        with pytest.raises(dab.DabhipError):
            call()
    edi.close()
    for args in ((0,), (1, 3), (1, -1), (1, 2, 6), (1, 2, -1), (1, 2, 0, 63), (1, 1, 0, 1473), (1, 0, 0, 1400, 65536), (1, 0, 0, 1400, -1)):
        with pytest.raises(dab.DabhipError):
            dab.Edi(*args)
    dab.Edi(1, 0, 9, 5).close()                                        # mode 0 takes no notice of recover and max_frag
    dab.Edi(1, 1, 9, 64).close()


# ---- end to end: modulated captures through the decoder and the stage ----------------------------------------------------------------------------
def test_end_to_end_from_iq_through_the_engine_on_device_frames():
    ntf = 24
    cfgs = [dab.synth_preset(0, seed=810 + b, cif_count0=(4990 + 1200 * b) % 5000, skip_samples=7000 * b) for b in range(2)]
    eng = dab.Engine(0)
    assert eng.decode([dab.synth_generate(c, ntf) for c in cfgs]) > 0
    ptr, total = eng.eti_device_ptr()
    counts = [eng.eti_count(b) for b in range(2)]
    assert sum(counts) == total and min(counts) >= 20
    edi = dab.Edi(2, dab.EDI_PFT_FEC, 2, 1400)
    assert edi.push((ptr, counts)) > 0
    for b in range(2):
        frames = list(eng.eti(b))
        assert all(m.accepted(f) is not None for f in frames)
        fields = _unpacks_to(edi.data(b), 2, frames)
        assert len(fields) == counts[b] and all(x["ficf"] == 1 and x["nst"] == cfgs[b].nsub for x in fields)
        st = m.Stream(2, 2, 1400)
        data, recs = st.push(frames)
        assert (edi.data(b) == data).all() and _recs(edi, b, 0) == recs and list(edi.stats(b)) == st.stat_list()
    edi.close()


def test_cli_dab2eti_pipe_eti2edi(tmp_path):
    here = os.path.dirname(dab.LIB_PATH)
    cfg = dab.synth_preset(0, seed=77, cif_count0=4995)
    cap = tmp_path / "cap.cu8"
    dab.synth_generate(cfg, 24).tofile(cap)
    eti = subprocess.run([os.path.join(here, "dab2eti-hip"), str(cap)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True, timeout=300).stdout
    frames = list(np.frombuffer(eti, np.uint8).reshape(-1, m.ETI_BYTES))
    assert len(frames) >= 20
    cmd = "set -o pipefail; '%s' '%s' | '%s' %s" % (os.path.join(here, "dab2eti-hip"), cap, os.path.join(here, "eti2edi"), "%s")
    for flags, (mode, recover, max_frag, seq0) in (("--fec 2", (2, 2, 1400, 0)), ("--pft --max-frag 255 --seq0 65530", (1, 0, 255, 65530)), ("-", (0, 0, 1400, 0))):
        run = subprocess.run(["bash", "-c", cmd % flags], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert run.returncode == 0, run.stderr
        st = m.Stream(mode, recover, max_frag, seq0)
        want, recs = st.push(frames)
        assert run.stdout == want.tobytes(), flags
        assert b"eti2edi: %d frames (0 skipped, 0 without FIC), %d packets, %d bytes" % (len(frames), len(recs), want.size) in run.stderr, run.stderr
    path = tmp_path / "in.eti"
    np.concatenate(frames).tofile(path)
    run = subprocess.run([os.path.join(here, "eti2edi"), "--fec", "2", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert run.returncode == 0 and run.stdout == m.pack(frames, 2, 2, 1400)[0].tobytes(), run.stderr
    for bad in (["--fec", "6"], ["--pft", "--fec", "1"], ["--max-frag", "63"], ["--nonsense"], ["a", "b"]):
        run = subprocess.run([os.path.join(here, "eti2edi")] + bad, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert run.returncode == 1 and run.stderr.startswith(b"Usage: eti2edi"), bad
