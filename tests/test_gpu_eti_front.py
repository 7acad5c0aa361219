"""What the five stages of ETI frames (DabPlus, Packet, Ts, Dir, Edi) have in common in front of their kernels (csrc/eti_push.hpp,
csrc/stage_frame.hpp, csrc/eti_lanes.hpp): the texts of their refusals, word for word, and ragged streams -- counts [0, n, m] -- pushed once
from host memory and once from device memory at an address that is no multiple of 16, which must give the same records, bytes and counters,
those of each stage's CPU model (the packet stage has that in test_gpu_packet.py::test_ways_frames_arrive_and_many_lanes: streams of 0, 1, 2
and more frames from host, device and odd device addresses against the model).  The refusals use no device memory beyond a handle's own."""
import ctypes as C

import numpy as np
import pytest

import dabplus_model
import dabtools_amd as dab
import dir_cases
import edi_cases
import test_gpu_dabplus as t_dabplus
import test_gpu_dir as t_dir
import test_gpu_edi as t_edi
import test_gpu_ts as t_ts
import ts_cases

pytestmark = pytest.mark.gpu

# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def _new(stage, nstreams=2):
    return {"dabplus": lambda: dab.DabPlus(nstreams, [1, 2]), "packet": lambda: dab.Packet(nstreams, [1, 2], [1, 0]), "ts": lambda: dab.Ts(nstreams, [1, 2]),
            "dir": lambda: dab.Dir(nstreams), "edi": lambda: dab.Edi(nstreams)}[stage]()


BOUND = {"dabplus": 1 << 24, "packet": 1 << 16, "ts": 1 << 16, "dir": 1 << 16, "edi": 1 << 17}
STAGES = tuple(BOUND)
LANE_STAGES = ("dabplus", "packet", "ts")


def _refused(result, text):
    assert result is None or result < 0, result
    assert dab.last_error() == text, (dab.last_error(), text)


def _raises(call, text):
    with pytest.raises(dab.DabhipError):
        call()
    assert dab.last_error() == text, (dab.last_error(), text)


@pytest.mark.parametrize("stage", STAGES)
def test_push_refusals_word_for_word(stage):
    h = _new(stage)
    push = getattr(dab.lib(), "dabhip_%s_push" % stage)
    who = stage + "_push: "
    counts = lambda *c: (C.c_int64 * 2)(*c)
    some = np.zeros(16, np.uint8).ctypes.data                         # never read: every call below is refused before
    _refused(push(None, some, counts(0, 0), 0), who + "null argument")
    _refused(push(h._h, some, None, 0), who + "null argument")
    for on_device in (0, 1):
        _refused(push(h._h, some, counts(0, -1), on_device), who + "bad frame count")
        _refused(push(h._h, some, counts(BOUND[stage] + 1, 0), on_device), who + "bad frame count")
        _refused(push(h._h, None, counts(0, BOUND[stage] + 1), on_device), who + "bad frame count")
        _refused(push(h._h, None, counts(0, 1), on_device), who + "null frames")
        if stage in ("dir", "edi"):                                   # each count legal, together one too many: the total is looked at before the frames
            _refused(push(h._h, None, counts(BOUND[stage], 1), on_device), who + "too many frames for one push")
            _refused(push(h._h, None, counts(1, BOUND[stage]), on_device), who + "too many frames for one push")
    assert push(h._h, None, counts(0, 0), 0) == 0                     # nothing to read: no pointer is needed
    _raises(lambda: h.push(np.zeros(0, np.uint8), [-1, 0]), who + "bad frame count")
    h.close()


@pytest.mark.parametrize("stage", STAGES)
def test_create_refusals_word_for_word(stage):
    who = stage + "_create: "
    _raises(lambda: _new(stage, 0), who + "bad arguments")
    _raises(lambda: _new(stage, -1), who + "bad arguments")
    made = {"dabplus": lambda ids, dev=0: dab.DabPlus(1, ids, dev), "packet": lambda ids, dev=0: dab.Packet(1, ids, [0] * len(ids), dev),
            "ts": lambda ids, dev=0: dab.Ts(1, ids, dev), "dir": lambda ids, dev=0: dab.Dir(1, dev), "edi": lambda ids, dev=0: dab.Edi(1, device=dev)}[stage]
    ndev = dab.lib().dabhip_device_count()
    for dev in (-1, ndev):
        _raises(lambda: made([1], dev), who + "device index out of range")
    if stage not in LANE_STAGES:
        return
    _raises(lambda: made([]), who + "bad arguments")
    _raises(lambda: made(list(range(64)) + [0]), who + "bad arguments")                     # 65 sub-channels
    _raises(lambda: made([3, 64]), who + "SubChId out of range")
    _raises(lambda: made([-1]), who + "SubChId out of range")
    create = getattr(dab.lib(), "dabhip_%s_create" % stage)
    ids = (C.c_int32 * 64)(*range(64))
    flags = np.zeros(64, np.uint8)
    extra = (flags.ctypes.data_as(C.POINTER(C.c_uint8)),) if stage == "packet" else ()
    assert not create(0, 1, None, *extra, 1) and dab.last_error() == who + "bad arguments"
    if stage == "packet":
        assert not create(0, 1, ids, None, 1) and dab.last_error() == who + "bad arguments"
    if stage != "dabplus":                                            # refused before anything is allocated
        ceiling = {"packet": 1 << 24, "ts": 1 << 18}[stage]
        assert not create(0, ceiling // 64 + 1, ids, *extra, 64) and dab.last_error() == who + "too many (stream, sub-channel) pairs"


@pytest.mark.parametrize("stage", STAGES)
def test_query_refusals_word_for_word(stage):
    h = _new(stage)
    if stage in LANE_STAGES:
        text = stage + ": no such stream / sub-channel"
        queries = [h.superframes, h.data, h.au_bytes, h.stats] if stage == "dabplus" else [h.records, h.data, h.stats]
        for q in queries:
            for at in ((2, 0), (-1, 0), (0, 2), (0, -1)):
                _raises(lambda: q(*at), text)
    else:
        text = stage + ": no such stream"
        queries = [h.stats, h.reset] + ([h.records, h.data] if stage == "edi" else [h.ensemble, h.subchannels, h.services, h.packet_components, h.complete])
        for q in queries:
            for at in (2, -1):
                _raises(lambda: q(at), text)
    h.close()


# ---- ragged streams, from the host and from an odd device address ---------------------------------------------------------------------------------
def _flat(streams):
    parts = [np.asarray(f, np.uint8).reshape(-1) for frames in streams for f in frames]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def _dabplus_streams():
    rng = np.random.default_rng(5)
    ids = [3, 9]
    streams = [[]] + [t_dabplus._frames(7 * nsf, [(scid, t_dabplus._protected_superframes(rng, s, nsf)) for scid, s in zip(ids, (1, 2))]) for nsf in (1, 2)]
    return ids, streams


def test_dabplus_ragged_streams_host_and_unaligned_device():
    """Streams of 0, 5 and 10 frames (0, 1 and 2 superframes) of two sub-channels."""
    ids, streams = _dabplus_streams()
    assert [len(f) for f in streams] == [0, 5, 10]
    flat, counts = _flat(streams), [len(f) for f in streams]
    buf = dab.DeviceBuffer(flat.size + 16)
    buf.upload(np.concatenate([np.zeros(1, np.uint8), flat]))
    assert buf.ptr % 16 == 0
    got = []
    for how in ("host", "device+1"):
        dp = dab.DabPlus(3, ids)
        assert (dp.push(flat, counts) if how == "host" else dp.push((buf.ptr + 1, counts))) == 6
        got.append({(b, q): (t_dabplus._gpu_lane(dp, b, q), list(dp.stats(b, q))) for b in range(3) for q in range(2)})
        dp.close()
    buf.free()
    for b, frames in enumerate(streams):
        for q, scid in enumerate(ids):
            sm = dabplus_model.SyncModel(scid)
            want = dabplus_model.stage(sm, frames)
            assert len(want) == (0, 1, 2)[b]
            for how, g in zip(("host", "device+1"), got):
                (recs, data, aus), stats = g[b, q]
                t_dabplus._assert_lane_equal(recs, data, aus, want, (how, b, scid))
                assert stats == t_dabplus._model_stats(want, sm.losses), (how, b, scid)
            (hr, hd, ha), (dr, dd, da) = got[0][b, q][0], got[1][b, q][0]
            assert hr.tobytes() == dr.tobytes() and hd.tobytes() == dd.tobytes() and ha == da and got[0][b, q][1] == got[1][b, q][1]


def _ts_streams():
    rng = np.random.default_rng(12)
    streams = [[]]
    for stl, nframes in ((204, 2), (51, 7)):
        stream = ts_cases.clean_stream(rng, nframes * 8 * stl, 100)[0]
        streams.append(ts_cases.frames_of_bytes(3, [(5, stl, stream)]))
    return [5], streams


def test_ts_ragged_streams_host_and_unaligned_device():
    """Streams of 0, 2 and 7 frames at 8 and 2 slots per frame: each just long enough for the run of five sync bytes and a few packets."""
    ids, streams = _ts_streams()
    assert [len(f) for f in streams] == [0, 2, 7]
    want, stats = t_ts._expect(streams, ids)
    assert not want[0, 0][0] and len(want[1, 0][0]) > 0 and len(want[2, 0][0]) > 0
    got = []
    for how in ("host", "device+1"):
        ts = dab.Ts(3, ids)
        got.append(t_ts._run(ts, streams, 1, None, how)[0])
        t_ts._assert_equal(ts, got[-1], want, stats, how)
        got[-1] = {k: (ts.records(*k).tobytes(), d.tobytes(), list(ts.stats(*k))) for k, (r, d) in got[-1].items()}
        ts.close()
    assert got[0] == got[1]


def test_dir_ragged_streams_host_and_unaligned_device():
    """Streams of 0, 1 and 3 frames of the rich carousel."""
    streams = [t_dir._rich(n, 40 + n) for n in (0, 1, 3)]
    models = t_dir._models(streams)
    assert models[0].good == 0 and models[1].good > 0 and models[2].good > 0
    got = []
    for how in ("host", "device+1"):
        d = dab.Dir(3)
        assert t_dir._push(d, streams, None, how) == sum(m.good for m in models)
        for b, m in enumerate(models):
            t_dir._same(d, b, m)
        got.append([(dir_cases.gpu_tuples(d, b), d.stats(b).tolist(), d.ensemble(b).tobytes(), d.subchannels(b).tobytes(), d.services(b).tobytes(),
                     d.packet_components(b).tobytes()) for b in range(3)])
        d.close()
    assert got[0] == got[1]


def test_edi_ragged_streams_host_and_unaligned_device():
    """Streams of 0, 1 and 2 small frames, as AF packets and as protected fragments."""
    rng = np.random.default_rng(3)
    streams = [[], [edi_cases.small_frame(rng, 249)], [edi_cases.small_frame(rng, 10 + i) for i in range(2)]]
    for mode, recover, max_frag in ((0, 0, 1400), (2, 2, 255)):
        want, stats = t_edi._expect(streams, mode, recover, max_frag)
        assert [len(want[b][1]) > 0 for b in range(3)] == [False, True, True]
        got = []
        for how in ("host", "device+1"):
            edi = dab.Edi(3, mode, recover, max_frag)
            g, total = t_edi._run(edi, streams, None, how)
            assert total == sum(len(want[b][1]) for b in want)
            t_edi._assert_equal(edi, g, want, stats, (mode, how))
            got.append({b: (d.tobytes(), r, edi.records(b).tobytes(), list(edi.stats(b))) for b, (d, r) in g.items()})
            edi.close()
        assert got[0] == got[1]
