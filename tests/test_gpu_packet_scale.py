"""The packet-mode kernels (k_packet.hip through Packet.push) at the shapes test_gpu_packet.py does not reach, bit for bit against the model of
packet_model.py (records, useful bytes, the eight statistics):

  rates    9, 16, 17, 102, 103, 104, 206 and 251 cells per ETI frame: the sync kernel's groups of eight headers past the first and the partial last
           group; from 103 on a whole FEC frame or several per ETI frame, units that begin and end inside one frame, the search after a third miss
           through the frame, earlier frames of the push and the carry
  lanes    1023, 1024, 1025, 2048, 2049 and 3073 (stream, sub-channel) pairs: the scan kernel's 1, 2, 3 and 4 lanes per thread, threads without a
           lane, bases handed from lane to lane inside a thread; the search for a cell's unit over thousands of units
  pushes   64 ETI frames at 251 cells each in one push, about 156 units in one lane: the slots packet.cpp plans per lane

Every input is legal by dabhip.h."""
import numpy as np
import pytest

import dabtools_amd as dab
import packet_cases as cs
import packet_model as m
import test_gpu_packet as base

pytestmark = pytest.mark.gpu

RATES = (9, 16, 17, 102, 103, 104, 206, 251)


def _dirty(frame, rng, nwords, most=10):
    """1 .. most wrong bytes on each of nwords code words of an FEC frame, in place (past 8 the word is left as received, or miscorrected)."""
    for r in rng.choice(m.ROWS, nwords, replace=False):
        err = np.zeros(m.N, np.uint8)
        ne = int(rng.integers(1, most + 1))
        err[rng.choice(m.N, ne, replace=False)] = rng.integers(1, 256, ne)
        cs.add_error(frame, int(r), err)
    return frame


def _stat(stats, key):
    return dict(zip(m.STATS, stats[key]))


# ---- a. every rate ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", RATES)
def test_every_rate(s):
    """One FEC lane that starts inside an FEC frame, three dirty code words in every frame; next to it (where it fits) a lane without FEC."""
    rng = np.random.default_rng(1000 + s)
    src = cs.TableSource(rng)
    nfr = 6 if s < 100 else 38
    # s = 104: the first cells of two units share an ETI frame only when a unit begins on the frame's first cell, which one of the 38 does when the
    # first whole FEC frame begins within 36 cells of the stream's start
    phase = int(rng.integers(70, 103)) if s == 104 else int(rng.integers(1, 103))
    first = m.FRAME_CELLS - phase                                  # the cell the first whole FEC frame begins at
    n_eti = -(-(first + m.FRAME_CELLS * nfr) // s)
    whole = (n_eti * s - first) // m.FRAME_CELLS
    assert nfr <= whole <= nfr + 2
    cells = np.concatenate([_dirty(m.fec_frame(src.unit()), rng, 3) for _ in range(whole + 2)])[phase * m.CELL:]
    subs, ids, fec = [(12, s, cells)], [12], [1]
    if s <= 206:
        plain_src = cs.TableSource(rng, addresses=(8, 9))
        plain = np.concatenate([plain_src.unit(3) for _ in range(n_eti)])
        plain[rng.choice(plain.size, 20, replace=False)] ^= 0x10
        subs, ids, fec = subs + [(40, 3, plain)], [12, 40], [1, 0]
    streams = [cs.frames_of_cells(200, subs, n_eti)]
    assert len(streams[0]) == n_eti
    want, stats = base._check(streams, ids, fec, [(None, "host"), (1, "host"), ("random", "host"), ("random", "device+1")], ("rate", s))
    st = _stat(stats, (0, 0))
    assert st["units"] == whole and st["rs_corrected_bytes"] > 0 and st["sync_losses"] == 0 and st["missed_frames"] == 0, st
    assert st["cells_skipped"] == first, st
    assert all(r[7] == m.FROM_FEC for r in want[0, 0][0]) and len(want[0, 0][0]) > 10 * whole
    in_frame = [(first + m.FRAME_CELLS * j) // s for j in range(whole)]
    if s >= 104:
        assert len(set(in_frame)) < len(in_frame), "no ETI frame holds the first cells of two units"
    if s < 103:
        assert all((first + m.FRAME_CELLS * j) // s < (first + m.FRAME_CELLS * (j + 1) - 1) // s for j in range(whole))     # a unit ends in a later frame
    if len(ids) == 2:
        plain_st = _stat(stats, (0, 1))
        assert plain_st["units"] == n_eti and plain_st["bad_cells"] > 0 and plain_st["packets"] > n_eti // 2, plain_st


# ---- b. the sync classes where frame borders fall inside ETI frames ----------------------------------------------------------------------------------
@pytest.mark.parametrize("s", (9, 103, 206))
def test_sync_classes_at_rate(s):
    """The crafted cell streams of packet_cases.sync_streams(): at 9 cells per frame and pushes of one frame the search after the third miss reads
    103 cells of which 94 or more lie in the carry; at 206 it stays inside one ETI frame."""
    sync = cs.sync_streams()
    labels = sorted(sync)
    streams = [cs.frames_of_cells(5 * i, [(7, s, cs.sent_whole(sync[k][0], s))]) for i, k in enumerate(labels)]
    assert all(len(f) * s * m.CELL >= len(sync[k][0]) for f, k in zip(streams, labels))        # every crafted cell is sent
    want, stats = base._check(streams, [7], [1], [(None, "host"), (1, "host"), ("random", "device")], ("sync", s))
    for i, k in enumerate(labels):
        st = _stat(stats, (i, 0))
        for name, v in sync[k][1].items():
            if name != "units":
                assert st[name] == v, (k, s, name, st)
            else:
                assert st[name] >= v, (k, s, name, st)              # (good frames follow the crafted cells up to a whole ETI frame)


# ---- c. broken streams at a high rate --------------------------------------------------------------------------------------------------------------
def test_broken_streams_at_104_cells_per_frame():
    """The five bad frames of test_broken_streams_and_an_id_listed_twice at STL 312, put where a unit is in progress (every place but a multiple of
    103 frames): after 5 frames, and after 7, which with pushes of 4 frames is behind three units of the same push."""
    rng = np.random.default_rng(6)
    src = cs.TableSource(rng)
    s, nfec = 104, 14
    cells = np.concatenate([m.fec_frame(src.unit()) for _ in range(nfec)])
    frames = cs.frames_of_cells(0, [(7, s, cells)])
    nf = len(frames)
    assert nf == nfec * m.FRAME_CELLS // s == 13
    one = s * m.CELL
    bad = {
        "absent": cs.raw_frame(9, [(8, 3 * s, None)]),
        "another STL": cs.raw_frame(9, [(7, 3 * s + 3, cells[:one + m.CELL])]),
        "STL 313": cs.raw_frame(9, [(7, 3 * s + 1, None)]),
        "past the frame": cs.raw_frame(9, [(3, 765, None), (7, 3 * s, None)]),
        "first of two": cs.raw_frame(9, [(7, 3 * s + 1, None), (7, 3 * s, cells[:one])]),
    }
    labels = sorted(bad)
    places = (5, 7)
    streams = [frames[:p] + [bad[k]] + frames[p:] for p in places for k in labels]
    want, stats = base._check(streams, [7, 9], [1, 0], [(None, "host"), (4, "host"), (1, "device"), ("random", "host")], "broken at 104")
    for i, (p, k) in enumerate((p, k) for p in places for k in labels):
        st = _stat(stats, (i, 0))
        # p frames give p units and leave p cells, dropped at the break.  The stream starts anew at cell p of an FEC frame, whose other 103 - p cells
        # go by before sync; whole frames from there on.  "another STL" carries 105 cells of its own, a whole FEC frame and 2 cells: one more unit,
        # and a second break (of a synced lane) in front of the frame behind it.
        more = k == "another STL"
        after = (s * (nf - p) - (m.FRAME_CELLS - p)) // m.FRAME_CELLS
        assert st["units"] == p + after + more and st["sync_losses"] == 1 + more and st["cells_skipped"] == p + (m.FRAME_CELLS - p) + 2 * more, (p, k, st)
        assert st["missed_frames"] == 0 and st["bad_cells"] == 0 and stats[i, 1][0] == 0, (p, k, st)
    with_four = [(p // 4 * 4, p) for p in places]
    assert any((p - a) * s // m.FRAME_CELLS >= 2 for a, p in with_four)      # two units out of the push's frames in front of the bad one


# ---- d. lanes --------------------------------------------------------------------------------------------------------------------------------------
POOL = 13                                                          # contents; a prime: coprime to 64 and to 1, 2, 3 and 4 lanes per scan thread
LENGTHS = (70, 0, 35)                                              # ETI frames per stream, from the last stream backwards
_pool = {}


def _contents():
    """[(cells per frame, cell bytes or None: the id is absent from every STC)], 70 frames of each."""
    if "contents" in _pool:
        return _pool["contents"]
    rng = np.random.default_rng(13)
    longest = max(LENGTHS)

    def fec(s, phase, nerr):
        src = cs.TableSource(rng, addresses=(3 + s, 700 + phase))
        c = np.concatenate([m.fec_frame(src.unit()) for _ in range(longest * s // m.FRAME_CELLS + 2)])[phase * m.CELL:][:longest * s * m.CELL].copy()
        c.reshape(-1, m.CELL)[:, 2:][tuple(rng.integers(0, [c.size // m.CELL, m.CELL - 2], (nerr, 2)).T)] ^= rng.integers(1, 256, nerr).astype(np.uint8)
        return s, c

    def plain(s, nerr):
        src = cs.TableSource(rng, addresses=(20 + s, 21))
        c = np.concatenate([src.unit(s) for _ in range(longest)])
        c[rng.choice(c.size, nerr, replace=False)] ^= 0x10
        return s, c

    out = [fec(3, 0, 12), fec(2, 11, 9), fec(1, 0, 3), plain(3, 0), (3, None), fec(3, 50, 30), plain(1, 4), fec(2, 0, 0), fec(3, 3, 60), plain(2, 9),
           fec(1, 99, 2), fec(3, 0, 5), plain(3, 30)]
    assert len(out) == POOL
    _pool["contents"] = out
    return out


def _lane_expectation(content, fec, nframes):
    """The model over the first nframes frames of a content in a lane with or without FEC, once: (records, bytes, statistics)"""
    key = (content, fec, nframes)
    if key not in _pool:
        s, c = _contents()[content]
        frames = cs.frames_of_cells(0, [(5, s, c)], nframes) if c is not None and nframes else [cs.raw_frame(f, [(6, 9, None)]) for f in range(nframes)]
        lane = m.Lane(5, fec)
        recs, data = lane.push(frames)
        _pool[key] = (recs, np.concatenate(data) if data else np.zeros(0, np.uint8), lane.stat_list())
    return _pool[key]


@pytest.mark.parametrize("nstreams,nsub", ((33, 31), (16, 64), (25, 41), (32, 64), (683, 3), (439, 7)))
def test_lanes(nstreams, nsub):
    """Lane l = stream x nsub + sub-channel, counted from the last lane backwards, holds content l mod 13 (FEC at 1, 2 and 3 cells per frame with
    errors, lanes without FEC, an id no STC lists), so neighbours never hold the same; every third sub-channel is decoded without FEC whatever it
    holds; the streams have 70, 0, 35, 70, ... frames from the last backwards.  Every lane is held to the model's records, bytes and statistics
    for what it was sent."""
    nlanes = nstreams * nsub
    assert nlanes in (1023, 1024, 1025, 2048, 2049, 3073)
    contents = _contents()
    ids = list(range(nsub))
    fec = [0 if q % 3 == 2 else 1 for q in range(nsub)]
    streams, want, stats = [], {}, {}
    for b in range(nstreams):
        n = LENGTHS[(nstreams - 1 - b) % 3]
        held = [(nlanes - 1 - b * nsub - q) % POOL for q in range(nsub)]
        streams.append([cs.raw_frame(b + f, [(q, 3 * contents[c][0], contents[c][1][f * 24 * contents[c][0]:(f + 1) * 24 * contents[c][0]])
                                             for q, c in enumerate(held) if contents[c][1] is not None]) for f in range(n)])
        for q, c in enumerate(held):
            recs, data, st = _lane_expectation(c, fec[q], n)
            want[b, q], stats[b, q] = (recs, data), st
    units = [stats[b, q][0] for b in range(nstreams) for q in range(nsub)]
    assert len(set(units)) >= 3 and 0 in units and units[-1] > 0, sorted(set(units))
    # The scan kernel gives thread t the lanes t chunk .. t chunk + chunk - 1.  Streams without frames and the lanes that never sync leave runs of
    # empty lanes, so not every border between two threads can have units on both sides; many do, others have none on one side or on both, and
    # where a thread has several lanes some threads hand a base on from one lane with units to the next
    chunk = (nlanes + 1023) // 1024
    borders = range(chunk, nlanes, chunk)
    both = sum(1 for a in borders if units[a - 1] > 0 and units[a] > 0)
    assert both >= 8 and any(units[a - 1] == 0 for a in borders) and any(units[a] == 0 for a in borders), (both, len(borders))
    if chunk > 1:
        assert sum(1 for a in range(0, nlanes - 1, chunk) if units[a] > 0 and units[a + 1] > 0) >= 8
    assert sum(units) > 2 * nlanes
    for chunk_frames, how in ((None, "host"), (9, "device")):
        pk = dab.Packet(nstreams, ids, fec)
        got = base._run(pk, streams, nsub, chunk_frames, how)
        base._assert_equal(pk, got, want, stats, ("lanes", nlanes, chunk_frames, how))
        pk.close()


# ---- e. a long push --------------------------------------------------------------------------------------------------------------------------------
def test_long_push_at_251_cells_per_frame():
    """What eti2pkt hands over at most, 64 ETI frames, at the highest rate: 155 units of one lane in one push; two dirty code words in every FEC
    frame.  A lane without FEC rides in a second stream that has no frame in that push."""
    rng = np.random.default_rng(251)
    src = cs.TableSource(rng)
    s, n_eti = 251, 66
    cells = np.concatenate([_dirty(m.fec_frame(src.unit()), rng, 2, most=8) for _ in range(n_eti * s // m.FRAME_CELLS + 1)])
    plain_src = cs.TableSource(rng, addresses=(8, 9))
    plain = np.concatenate([plain_src.unit(3) for _ in range(5)])
    plain[rng.choice(plain.size, 6, replace=False)] ^= 0x10
    streams = [cs.frames_of_cells(100, [(12, s, cells)], n_eti), cs.frames_of_cells(7, [(40, 3, plain)])]
    assert [len(f) for f in streams] == [n_eti, 5]
    ids, fec = [12, 40], [1, 0]
    want, stats = base._expect(streams, ids, fec)
    st = _stat(stats, (0, 0))
    assert st["units"] == n_eti * s // m.FRAME_CELLS == 160 and st["rs_corrected_bytes"] >= 2 * 160 and st["rs_failed_codewords"] == 0 and st["bad_cells"] == 0, st
    assert stats[1, 1][0] == 5 and stats[0, 1][0] == 0 and stats[1, 0][0] == 0
    # one handle: 64 frames of the first stream alone, then the rest with the second stream's
    pk = dab.Packet(2, ids, fec)
    got = {k: ([], []) for k in want}
    for counts in ((64, 0), (n_eti - 64, 5)):
        parts = [streams[0][:64] if counts[0] == 64 else streams[0][64:], streams[1][:counts[1]]]
        pk.push(np.concatenate([np.asarray(f, np.uint8) for p in parts for f in p]), list(counts))
        if counts[0] == 64:
            first = dict(zip(dab.PACKET_STATS, pk.stats(0, 0)))
            assert first["units"] == 64 * s // m.FRAME_CELLS == 155 >= 150, first
        for key, (r, d) in got.items():
            rr, dd = base._gpu_lane(pk, *key)
            r += rr
            d.append(dd)
    base._assert_equal(pk, {k: (r, np.concatenate(d)) for k, (r, d) in got.items()}, want, stats, "long push")
    pk.close()
    # a second handle: the same frames in pushes of 64, both streams from their first frames on
    pk = dab.Packet(2, ids, fec)
    base._assert_equal(pk, base._run(pk, streams, 2, 64, "device"), want, stats, "pushes of 64")
    pk.close()
