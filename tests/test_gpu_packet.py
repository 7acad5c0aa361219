"""The packet-mode kernels (k_packet.hip through Packet.push) against the model of packet_model.py, bit for bit: records, useful bytes and
statistics.  ETI frames are built by hand from the model and the crafted classes of packet_cases.py: Reed-Solomon words at the decoder's edges,
cell streams at the edges of the FEC sync rule, broken streams, the walk's edges; with and without FEC in one handle; 1, 4 and 8 cells per ETI
frame (9 to 251, more than 1024 lanes and pushes of 64 frames: test_gpu_packet_scale.py); 5, 6 and 22 FEC frames per lane (60, 72 and 264 code words: across the wave and workgroup edges); every way frames arrive and any cutting
into pushes, pushes of 0 and 1 frame included; and the data groups of the library's host rule against what the source of the packets sent."""
import os
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import packet_cases as cs
import packet_model as m

pytestmark = pytest.mark.gpu


def _gpu_lane(pk, b, q):
    recs = pk.records(b, q)
    return [tuple(int(v) for v in r) for r in recs.tolist()], pk.data(b, q)


def _cuts(nframes, chunk, rng):
    """Frame counts of the pushes: fixed, or random with pushes of 0 and 1 frame among them."""
    if chunk is None:
        return [nframes]
    if chunk != "random":
        return [min(chunk, nframes - a) for a in range(0, nframes, chunk)] or [0]
    out, left = [0, 1], nframes - 1
    while left > 0:
        n = int(rng.choice([0, 1, 2, 5, 17, 60, 103, 200, 411]))
        out.append(min(n, left))
        left -= out[-1]
    return out if nframes > 0 else [0]


def _run(pk, streams, nsub, chunk=None, how="host", seed=0):
    """Push the streams in cuts (the same cut positions for every stream, scaled to its length) -> {(stream, sub): (records, bytes)}"""
    rng = np.random.default_rng(seed)
    longest = max(len(f) for f in streams)
    got = {(b, q): ([], []) for b in range(len(streams)) for q in range(nsub)}
    total, at = 0, 0
    for n in _cuts(longest, chunk, rng):
        parts = [f[at:at + n] for f in streams]
        at += n
        counts = [len(p) for p in parts]
        flat = np.concatenate([np.asarray(f, np.uint8).reshape(-1) for p in parts for f in p]) if sum(counts) else np.zeros(0, np.uint8)
        buf = None
        if how == "host":
            total += pk.push(flat, counts)
        else:
            off = 1 if how == "device+1" else 0
            buf = dab.DeviceBuffer(flat.size + 16)
            assert buf.ptr % 16 == 0
            buf.upload(np.concatenate([np.zeros(off, np.uint8), flat]))
            total += pk.push((buf.ptr + off, counts))
        for key, (r, d) in got.items():
            rr, dd = _gpu_lane(pk, *key)
            r += rr
            d.append(dd)
        if buf is not None:
            buf.free()
    assert total == sum(len(r) for r, _ in got.values())
    return {k: (r, np.concatenate(d)) for k, (r, d) in got.items()}


def _expect(streams, ids, fec):
    """The model over whole streams -> ({(stream, sub): (records, bytes)}, {(stream, sub): statistics})"""
    want, stats = {}, {}
    for b, frames in enumerate(streams):
        for q, (scid, f) in enumerate(zip(ids, fec)):
            lane = m.Lane(scid, f)
            recs, data = lane.push(frames)
            want[b, q] = (recs, np.concatenate(data) if data else np.zeros(0, np.uint8))
            stats[b, q] = lane.stat_list()
    return want, stats


def _assert_equal(pk, got, want, stats, ctx):
    for key, (recs, data) in want.items():
        grecs, gdata = got[key]
        assert len(grecs) == len(recs), (ctx, key, len(grecs), len(recs))
        for i, (a, b) in enumerate(zip(grecs, recs)):
            assert a == tuple(b), (ctx, key, i, a, b)
        assert gdata.size == data.size and (gdata == data).all(), (ctx, key)
        assert list(pk.stats(*key)) == stats[key], (ctx, key, list(pk.stats(*key)), stats[key])


def _check(streams, ids, fec, plans, ctx):
    want, stats = _expect(streams, ids, fec)
    for chunk, how in plans:
        pk = dab.Packet(len(streams), ids, fec)
        got = _run(pk, streams, len(ids), chunk, how, seed=len(streams))
        _assert_equal(pk, got, want, stats, (ctx, chunk, how))
        pk.close()
    return want, stats


def test_rs_classes_through_the_stage():
    """Every crafted word's error pattern on a code word of a frame of packets: a corrected word's packets pass their CRC, a word left as
    received (or a miscorrection that differs from the model's) shows in the records, the bytes and the counters."""
    rng = np.random.default_rng(41)
    cases = cs.rs_cases()
    patterns = cs.error_patterns(cases)
    assert len(patterns) > 350
    frames = cs.frames_with_errors(cs.TableSource(rng), patterns)
    pad = [m.make_packet(1, 0, 3, 0, 0, b"")] * (-len(frames) * 103 % 8)                # up to whole ETI frames of 8 cells
    cells = np.concatenate(frames + pad)
    for s in (8, 1):
        streams = [cs.frames_of_cells(11, [(6, s, cells)])]
        want, stats = _check(streams, [6], [1], [(None, "host"), (100, "device")], ("rs", s))
        st = dict(zip(m.STATS, stats[0, 0]))
        # by construction: every word of classes e8, e1, parity and miscorrect is corrected, every word of class shortened fails
        assert st["rs_failed_codewords"] >= 10 + 290 and st["rs_corrected_bytes"] >= 12 * 8 + 5 + 13 + 8 * 8, st
        assert st["units"] == len(frames) == -(-len(patterns) // 12), st


@pytest.mark.parametrize("s", (1, 4, 8))
@pytest.mark.parametrize("nframes", (5, 6, 22))
def test_frames_per_lane_and_cells_per_eti_frame(nframes, s):
    """One FEC lane of nframes FEC frames at s cells per ETI frame (s = 1: a frame spans 103 ETI frames), dirty code words in every frame, next
    to a lane without FEC in the same handle; one push, random cuts with pushes of 0 and 1 frame, device frames."""
    rng = np.random.default_rng(100 * nframes + s)
    src = cs.TableSource(rng)
    frames = []
    for _ in range(nframes):
        f = m.fec_frame(src.unit())
        for r in rng.choice(12, 5, replace=False):
            err = np.zeros(m.N, np.uint8)
            ne = int(rng.integers(1, 11))
            err[rng.choice(m.N, ne, replace=False)] = rng.integers(1, 256, ne)
            cs.add_error(f, int(r), err)
        frames.append(f)
    cells = np.concatenate(frames + [m.fec_frame(src.unit())[:(-nframes * 103) % s * m.CELL]])      # filled up to whole ETI frames
    n_eti = len(cells) // (m.CELL * s)
    plain_src = cs.TableSource(rng, addresses=(8, 9))
    plain = np.concatenate([plain_src.unit(3) for _ in range(n_eti)])
    plain[rng.choice(plain.size, 20, replace=False)] ^= 0x10
    streams = [cs.frames_of_cells(200, [(12, s, cells), (40, 3, plain)])]
    assert len(streams[0]) == n_eti
    want, stats = _check(streams, [12, 40], [1, 0], [(None, "host"), ("random", "host"), ("random", "device+1")], (nframes, s))
    st = dict(zip(m.STATS, stats[0, 0]))
    assert st["units"] == nframes and st["rs_corrected_bytes"] > 0 and st["sync_losses"] == 0 and st["cells_skipped"] == 0, st
    plain_st = dict(zip(m.STATS, stats[0, 1]))
    assert plain_st["units"] == n_eti and plain_st["bad_cells"] > 0 and plain_st["packets"] > n_eti // 2, plain_st
    assert all(r[7] == m.FROM_FEC for r in want[0, 0][0]) and all(r[7] == 0 for r in want[0, 1][0])


def test_sync_classes_through_the_stage():
    sync = cs.sync_streams()
    labels = sorted(sync)
    for s in (1, 4):
        streams = [cs.frames_of_cells(5 * i, [(7, s, sync[k][0])]) for i, k in enumerate(labels)]
        want, stats = _check(streams, [7], [1], [(None, "host"), (50, "host"), ("random", "device"), (1, "host")] if s == 4 else [(None, "host"), (97, "device+1")], ("sync", s))
        for i, k in enumerate(labels):
            st = dict(zip(m.STATS, stats[i, 0]))
            for name, v in sync[k][1].items():
                if s == 1 or name != "units":
                    assert st[name] == v, (k, s, name, st)


def test_broken_streams_and_an_id_listed_twice():
    rng = np.random.default_rng(5)
    src = cs.TableSource(rng)
    cells = np.concatenate([m.fec_frame(src.unit()) for _ in range(6)])
    frames = cs.frames_of_cells(0, [(7, 2, cells)])
    twice_good = [cs.raw_frame(f[4], [(7, 6, cells[48 * i:48 * i + 48]), (9, 3, None), (7, 6, None)]) for i, f in enumerate(frames)]
    bad = {
        "absent": cs.raw_frame(9, [(8, 6, None)]),
        "another STL": cs.raw_frame(9, [(7, 9, cells[:72])]),
        "STL 7": cs.raw_frame(9, [(7, 7, None)]),
        "past the frame": cs.raw_frame(9, [(3, 765, None), (7, 6, None)]),
        "first of two": cs.raw_frame(9, [(7, 7, None), (7, 6, cells[:48])]),
    }
    labels = sorted(bad)
    streams = [frames[:130] + [bad[k]] + frames[130:] for k in labels] + [twice_good, frames[:40] + [bad["another STL"]] * 3 + frames[40:]]
    want, stats = _check(streams, [7, 9], [1, 0], [(None, "host"), (40, "host"), (131, "device"), ("random", "host")], "broken")
    for i, k in enumerate(labels):
        st = dict(zip(m.STATS, stats[i, 0]))
        assert st["sync_losses"] == 1 and st["units"] == 5 and st["cells_skipped"] == 54 + 49 + (3 if k == "another STL" else 0), (k, st)
    assert stats[len(labels), 0] == [6, 0, 0, 0] + stats[len(labels), 0][4:] and want[len(labels), 0][0], "the first entry of an id listed twice counts"
    assert stats[len(labels), 1][0] == len(frames)                     # sub-channel 9 rides along without FEC: one unit per frame


def test_walk_edges_through_the_stage():
    rng = np.random.default_rng(11)
    table, taken, bad = cs.walk_table(rng)
    streams = [cs.frames_of_cells(0, [(4, 1, m.fec_frame(table))]), cs.frames_of_cells(0, [(4, 94, table)]), cs.frames_of_cells(0, [(4, 5, table)])]
    for fec in (1, 0):
        want, stats = _check(streams, [4], [fec], [(None, "host"), (10, "device")], ("walk", fec))
        flag = m.FROM_FEC if fec else 0
        b = 0 if fec else 1
        assert [(r[0], r[1], r[2], r[7]) for r in want[b, 0][0]] == [(k, a, L, flag) for k, a, L in taken]
        assert stats[b, 0][4] == bad
    assert all(r[0] % 5 + r[2] <= 5 for r in want[2, 0][0])


def test_ways_frames_arrive_and_many_lanes():
    """30 streams x 3 sub-channels of different rates, lengths and start phases, errors in every lane; host, device and unaligned device frames;
    one push and cuts of 9 frames must all give the same."""
    rng = np.random.default_rng(77)
    ids, fec, rates = [3, 17, 62], [1, 0, 1], [2, 3, 5]
    streams = []
    for b in range(30):
        n_eti = (0, 1, 2, 40, 130, 150)[b % 6] if b % 6 < 3 else int(rng.integers(60, 160))
        subs = []
        for scid, f, s in zip(ids, fec, rates):
            src = cs.TableSource(rng, addresses=(1 + b, 700))
            need = n_eti * s + 103
            if f:
                cells = np.concatenate([m.fec_frame(src.unit()) for _ in range(need // 103 + 2)])[int(rng.integers(103)) * m.CELL:]
            else:
                cells = np.concatenate([src.unit(s) for _ in range(n_eti + 1)])
            cells = cells.copy()
            ne = int(rng.integers(0, 40))
            cells[rng.choice(cells.size, ne, replace=False)] ^= rng.integers(1, 256, ne).astype(np.uint8)
            subs.append((scid, s, cells))
        streams.append(cs.frames_of_cells(b, subs, n_eti) if n_eti else [])
    want, stats = _check(streams, ids, fec, [(None, "host"), (None, "device"), (9, "device+1"), (9, "host")], "lanes")
    total = np.sum([stats[k] for k in stats], axis=0)
    assert total[0] > 1000 and total[6] > 0 and total[3] > 0 and total[5] > 2500, total


def test_data_groups_of_the_stage_against_the_source():
    """Packets of a source of data groups through the stage (FEC, with errors the code corrects) and the library's host rule: every group the source
    completed comes out, byte for byte, in order."""
    rng = np.random.default_rng(91)
    src = cs.TableSource(rng)
    frames = []
    for _ in range(12):
        f = m.fec_frame(src.unit())
        for r in range(12):
            err = np.zeros(m.N, np.uint8)
            err[rng.choice(m.N, 8, replace=False)] = rng.integers(1, 256, 8)
            cs.add_error(f, r, err)
        frames.append(f)
    assert 12 * 103 % 6 == 0
    eti = cs.frames_of_cells(0, [(2, 6, np.concatenate(frames))])
    pk, groups, model = dab.Packet(1, [2], [1]), dab.PacketGroups(), m.Groups()
    got, lane = [], m.Lane(2, True)
    for a in range(0, len(eti), 25):
        pk.push(np.array(eti[a:a + 25]))
        got += groups.push(pk.records(0, 0), pk.data(0, 0))
    assert list(pk.stats(0, 0))[6:] == [12 * 12 * 8, 0]
    want = model.push(*lane.push(eti))
    assert len(got) == len(want) >= 20
    for (gr, gb), (wr, wb) in zip(got, want):
        assert (gb == wb).all() and all(int(gr[k]) == v for k, v in wr.items())
    assert len(want) == len(src.groups)
    for (gr, gb), (a, g) in zip(got, src.groups):
        assert int(gr["address"]) == a and (gb == g).all() and (not gr["crc_flag"] or gr["crc_ok"])
    assert list(groups.stats()) == model.stat_list() and groups.stats()[1] == 0
    pk.close()
    groups.close()


def test_stage_times_and_refusals():
    pk = dab.Packet(1, [1, 2], [1, 0])
    assert pk.push(np.zeros(0, np.uint8), [0]) == 0
    assert set(pk.stage_ms()) == {"locate", "sync", "gather", "rs", "cand", "walk", "carry"}
    with pytest.raises(dab.DabhipError):
        pk.records(1, 0)
    with pytest.raises(dab.DabhipError):
        pk.stats(0, 2)
    pk.close()
    with pytest.raises(dab.DabhipError):
        dab.Packet(1, [64], [0])
    with pytest.raises(dab.DabhipError):
        dab.Packet(0, [1], [0])


# ---- end to end: modulated captures through the decoder and the stage ----------------------------------------------------------------------------
def _truth_groups(cfg, slot, cifs):
    """What the modulator put into the units of a slot that lie whole in the logical CIFs `cifs` (consecutive): [(address, bytes)] by the model's
    walk and group rule over the modulator's own cells -- which test_packet_model.py holds against dabhip_synth_packet_group."""
    assert cifs == list(range(cifs[0], cifs[0] + len(cifs)))
    s = dab.synth_payload(cfg, 0, slot).size // 24
    out = []
    if cfg.packet_fec_slots >> slot & 1:
        first = -(-(cifs[0] * s - cfg.packet_phase) // 103)
        j = first
        while 103 * (j + 1) + cfg.packet_phase <= (cifs[-1] + 1) * s:
            out += cs.unit_groups(dab.synth_packet_cells(cfg, slot, 103 * j + cfg.packet_phase, 94))[1]
            j += 1
        return out, j - first
    for c in cifs:
        out += cs.unit_groups(dab.synth_packet_cells(cfg, slot, c * s, s))[1]
    return out, len(cifs)


def _cifs_of(cfg, frames, ntf):
    index = {dab.synth_fibs(cfg, c).tobytes(): c for c in range(4 * ntf)}
    return [index[f[12 + 4 * (f[5] & 0x7f):][:96].tobytes()] for f in frames]


def test_end_to_end_from_iq_through_the_engine_on_device_frames():
    ntf, cfgs = 40, []
    for b in range(2):
        cfg = dab.synth_preset(0, seed=900 + b, cif_count0=(2237 * b) % 5000, skip_samples=7000 * b)
        cfg.packet_slots = (1 << cfg.nsub) - 1
        cfg.packet_fec_slots = 0b110101010101
        cfg.packet_phase = 5 + 37 * b
        cfgs.append(cfg)
    nsub = cfgs[0].nsub
    ids = [cfgs[0].sub[k].id for k in range(nsub)]
    fec = [cfgs[0].packet_fec_slots >> k & 1 for k in range(nsub)]
    eng = dab.Engine(0)
    assert eng.decode([dab.synth_generate(c, ntf) for c in cfgs]) > 0
    ptr, total = eng.eti_device_ptr()
    counts = [eng.eti_count(b) for b in range(2)]
    assert sum(counts) == total and min(counts) >= 80
    pk = dab.Packet(2, ids, fec)
    assert pk.push((ptr, counts)) > 0
    units = 0
    for b, cfg in enumerate(cfgs):
        cifs = _cifs_of(cfg, eng.eti(b), ntf)
        for q in range(nsub):
            want, nunits = _truth_groups(cfg, q, cifs)
            groups = dab.PacketGroups()
            got = groups.push(pk.records(b, q), pk.data(b, q))
            st = dict(zip(dab.PACKET_STATS, pk.stats(b, q)))
            assert st["units"] == nunits and st["bad_cells"] == 0 and st["rs_failed_codewords"] == 0 and st["sync_losses"] == 0, (b, q, st, nunits)
            assert [(int(r["address"]), bytes(g)) for r, g in got] == [(a, bytes(g)) for a, g in want], (b, q)
            assert all(r["header_ok"] and r["crc_ok"] == r["crc_flag"] for r, _ in got)
            assert list(groups.stats())[1:] == [0, 0, 0]
            units += nunits if fec[q] else 0
            groups.close()
    assert units >= 80
    pk.close()


def test_cli_dab2eti_pipe_eti2pkt(tmp_path):
    here = os.path.dirname(dab.LIB_PATH)
    ntf = 30
    cfg = dab.synth_preset(0, seed=93, cif_count0=4990)
    cfg.packet_slots = (1 << cfg.nsub) - 1
    cfg.packet_fec_slots = 0b000000110011
    cfg.packet_phase = 60
    cap = tmp_path / "cap.cu8"
    dab.synth_generate(cfg, ntf).tofile(cap)
    eti = subprocess.run([os.path.join(here, "dab2eti-hip"), str(cap)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True).stdout
    frames = list(np.frombuffer(eti, np.uint8).reshape(-1, m.ETI_BYTES))
    cifs = _cifs_of(cfg, frames, ntf)
    for slot in (0, 5, 9):
        fec = cfg.packet_fec_slots >> slot & 1
        want, nunits = _truth_groups(cfg, slot, cifs)
        assert len(want) > 20
        cmd = "set -o pipefail; '%s' '%s' | '%s' %d%s%s" % (os.path.join(here, "dab2eti-hip"), cap, os.path.join(here, "eti2pkt"), cfg.sub[slot].id, " --fec" if fec else "", "%s")
        run = subprocess.run(["bash", "-c", cmd % ""], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert run.returncode == 0, run.stderr
        assert run.stdout == b"".join(bytes([a >> 8, a & 255, len(g) >> 8, len(g) & 255]) + bytes(g) for a, g in want), slot
        assert b"eti2pkt: %d frames" % len(frames) in run.stderr and b" %d units" % nunits in run.stderr and b"%d data groups (%d written)" % (len(want), len(want)) in run.stderr
        one = want[0][0]
        run = subprocess.run(["bash", "-c", cmd % (" --address %d" % one)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert run.returncode == 0 and run.stdout == b"".join(bytes([a >> 8, a & 255, len(g) >> 8, len(g) & 255]) + bytes(g) for a, g in want if a == one)
