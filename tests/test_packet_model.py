"""The packet-mode model (tests/packet_model.py) on the CPU: its RS(204,188) against long division and against the independent decoder of
rs204_reference.py on every crafted word, the FEC sync rule, the walk and the data-group rule on crafted inputs whose results the construction
fixes, independence of how a stream is cut into pushes, the host rule of the library (dabhip_packet_groups_*) against the model's, and
tests/host_sanitize/packet_units.cpp, a stand-alone program, under ASan + UBSan: the sync rule at every rate of RATES and the bound on a push's
units per lane (packet.cpp) as a property over every rate, carried count and push size."""
import os
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import packet_cases as cs
import packet_model as m
import rs204_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generator_and_parity_against_long_division():
    assert m.GEN == ref.GEN and len(m.GEN) == 17 and m.GEN[0] == 1
    for i in range(16):                                           # alpha^i is a root
        v = 0
        for c in m.GEN:
            v = ref.mul(v, ref.power(2, i)) ^ c
        assert v == 0, i
    rng = np.random.default_rng(1)
    for _ in range(20):
        data = rng.integers(0, 256, m.K, dtype=np.uint8)
        par = m.rs_parity(data)
        assert (par == ref.encode(data)).all()
        assert not any(ref.syndromes(np.concatenate([data, par])))


RS = cs.rs_cases()


@pytest.mark.parametrize("cls", sorted(RS))
def test_model_decoder_against_the_reference_on_every_word(cls):
    counts = {}
    for label, rx, want, n, err in RS[cls]:
        assert not any(ref.syndromes(rx ^ err)), (cls, label)
        a, na = m.rs_decode(rx)
        b, nb = ref.decode(rx)
        assert na == nb and (a == b).all(), (cls, label, na, nb)
        if n is not None:
            assert na == n and (a == want).all(), (cls, label, na, n)
        if na < 0:
            assert (a == rx).all(), (cls, label)
        counts[na] = counts.get(na, 0) + 1
    if cls == "beyond":
        assert len(RS[cls]) >= 300 and counts.get(-1, 0) >= 290, counts
    if cls == "shortened":
        assert counts == {-1: len(RS[cls])}, counts
    if cls == "e9":
        assert counts.get(-1, 0) >= 10, counts


def test_frame_layout_and_decode():
    rng = np.random.default_rng(3)
    table = rng.integers(0, 256, m.TABLE, dtype=np.uint8)
    frame = m.fec_frame(table).reshape(m.FRAME_CELLS, m.CELL)
    z = np.concatenate([table, m.table_parity(table)])
    for r in range(m.ROWS):
        assert not any(ref.syndromes(z[r::m.ROWS])), r
    for i in range(m.FEC_CELLS):
        assert m.fec_counter(frame[m.DATA_CELLS + i]) == i
        assert frame[m.DATA_CELLS + i, 0] >> 6 == 0 and (int(frame[m.DATA_CELLS + i, 0]) & 3) << 8 | int(frame[m.DATA_CELLS + i, 1]) == 1022
    assert (frame[m.DATA_CELLS:, 2:].reshape(-1)[192:] == 0).all()
    rx = frame.copy().reshape(-1)
    rx[0:8 * 12:12] ^= 0x5A                                       # 8 errors in code word 0
    rx[1:9 * 12:12] ^= 0xA5                                       # 9 in code word 1
    got, fixed, failed = m.decode_frame(rx)
    assert fixed == 8 and failed == 1
    assert (got.reshape(-1)[0::12] == table[0::12]).all() and (got.reshape(-1)[1::12] == rx[:m.TABLE][1::12]).all()


def _run(lane, frames, chunk=None):
    recs, data = [], []
    step = chunk or max(len(frames), 1)
    for a in range(0, max(len(frames), 1), step):
        r, d = lane.push(frames[a:a + step])
        recs += r
        data += d
    return recs, data


SYNC = cs.sync_streams()
# 9: the second group of eight headers; 102, 103, 104: a frame to an ETI frame, less and more; 206, 251: two frames and more to an ETI frame, 251 the
# most that fits behind the FIC bytes
RATES = (9, 16, 17, 102, 103, 104, 206, 251)
RATE_PLANS = tuple((s, chunk) for s in RATES for chunk in (None, 1))


@pytest.mark.parametrize("cls", sorted(SYNC))
def test_sync_rule_on_crafted_streams(cls):
    cells, want = SYNC[cls]
    results = []
    for s, chunk in ((1, None), (1, 50), (4, 7), (8, 1)) + RATE_PLANS:
        frames = cs.frames_of_cells(3, [(7, s, cs.sent_whole(cells, s) if s > 8 else cells)])
        lane = m.Lane(7, True)
        recs, data = _run(lane, frames, chunk)
        for k, v in want.items():
            if s == 1 or k != "units":                            # (with s > 1 the cells left over at the end may cost the last frame)
                assert lane.stats[k] == v, (cls, s, chunk, k, lane.stats)
            elif s > 8:                                           # (every cell was sent, and good frames behind them)
                assert lane.stats[k] >= v, (cls, s, chunk, k, lane.stats)
        assert lane.stats["rs_failed_codewords"] == 0 and lane.stats["rs_corrected_bytes"] == 0
        sent = len(frames) * s
        assert lane.stats["units"] * 103 + lane.stats["cells_skipped"] + len(lane.cells) == sent, (cls, s, chunk)
        assert len(lane.cells) <= m.CARRY
        if s == 1 or s > 8:
            results.append((recs, [bytes(d) for d in data], lane.stat_list()))
    assert all(a == b for a, b in zip(results[0::2], results[1::2])) and len(results) == 2 + len(RATE_PLANS)    # any cut gives the same
    if cls == "slip of 11 cells":
        assert lane.stats["units"] >= 6 and lane.stats["cells_skipped"] >= 92


def test_broken_streams():
    rng = np.random.default_rng(5)
    src = cs.TableSource(rng)
    cells = np.concatenate([m.fec_frame(src.unit()) for _ in range(6)])
    frames = cs.frames_of_cells(0, [(7, 2, cells)])
    assert len(frames) == 309
    absent = cs.raw_frame(9, [(8, 6, None)])
    other_stl = cs.raw_frame(9, [(7, 9, cells[:72])])
    odd_stl = cs.raw_frame(9, [(7, 7, None)])
    past = cs.raw_frame(9, [(3, 765, None), (7, 6, None)])
    twice = cs.raw_frame(9, [(7, 7, None), (7, 6, cells[:48])])
    for label, bad, extra_cells in (("absent", absent, 0), ("another STL", other_stl, 3), ("STL 7", odd_stl, 0), ("past the frame", past, 0), ("first of two", twice, 0)):
        lane = m.Lane(7, True)
        recs, _ = _run(lane, frames[:130] + [bad] + frames[130:], 40)
        # 260 cells: frames 0 and 1 decoded, 54 cells dropped at the break; then the stream starts anew in the middle of frame 2
        assert lane.stats["sync_losses"] == 1 and lane.stats["units"] == 2 + 3, (label, lane.stats)
        assert lane.stats["cells_skipped"] == 54 + extra_cells + 49, (label, lane.stats)
        assert lane.first + len(lane.cells) == 618 + extra_cells, label
    plain = m.Lane(7, False)
    recs, _ = _run(plain, frames[:10] + [absent] + frames[10:20], 3)
    assert plain.stats["units"] == 20 and plain.stats["sync_losses"] == 0 and plain.stats["cells_skipped"] == 0


def test_walk_edges():
    rng = np.random.default_rng(11)
    table, want, bad = cs.walk_table(rng)
    recs, data, nbad = m.walk(table, 1000, 0)
    assert [(r[0] - 1000, r[1], r[2]) for r in recs] == want and nbad == bad
    assert any(r[1] == 0 for r in recs)                           # padding packets are taken
    assert bytes(data[0]) == b"a good packet one cell later" and bytes(data[-1]) == b"last cell"
    for r, d in zip(recs, data):
        assert len(d) == r[6] <= 24 * r[2] - 5
    # through a lane, with and without FEC
    lane = m.Lane(4, True)
    got, _ = lane.push(cs.frames_of_cells(0, [(4, 1, m.fec_frame(table))]))
    assert [(r[0], r[1], r[2], r[7]) for r in got] == [(k, a, L, m.FROM_FEC) for k, a, L in want] and lane.stats["bad_cells"] == bad
    short = m.Lane(4, False)
    got, _ = short.push(cs.frames_of_cells(0, [(4, 94, table)]))
    assert [(r[0], r[1], r[2], r[7]) for r in got] == [(k, a, L, 0) for k, a, L in want]
    # the same cells 5 to an ETI frame: a packet that would cross a frame's end is not taken
    five = m.Lane(4, False)
    got, _ = five.push(cs.frames_of_cells(0, [(4, 5, table)]))
    assert all(r[0] % 5 + r[2] <= 5 for r in got) and 0 < len(got) < len(want)


def _groups_through(lib_side, recs, data, cut):
    got = []
    for a in range(0, len(recs), cut):
        r, d = recs[a:a + cut], data[a:a + cut]
        arr = np.array([tuple(x) for x in r], dtype=dab.PACKET_REC) if r else np.zeros(0, dab.PACKET_REC)
        got += lib_side.push(arr, np.concatenate(d) if d else np.zeros(0, np.uint8))
    return got


def _assert_groups_equal(got, want, ctx):
    assert len(got) == len(want), (ctx, len(got), len(want))
    for (gr, gb), (wr, wb) in zip(got, want):
        assert (np.asarray(gb) == wb).all(), ctx
        for k, v in wr.items():
            assert int(gr[k]) == v, (ctx, k, int(gr[k]), v)


def test_data_groups_from_a_source():
    rng = np.random.default_rng(21)
    src = cs.TableSource(rng)
    recs, data = [], []
    for u in range(40):
        r, d, bad = m.walk(src.unit(), 94 * u, 0)
        assert bad == 0
        recs += r
        data += d
    model = m.Groups()
    done = model.push(recs, data)
    assert len(done) == len(src.groups) >= 30 and model.stats["dropped"] == 0 and model.stats["crc_fails"] == 0
    for (g, b), (addr, truth) in zip(done, src.groups):
        assert g["address"] == addr and (b == truth).all() and g["header_ok"] and g["crc_ok"] == g["crc_flag"]
    flags = {(g["ext_flag"], g["crc_flag"], g["seg_flag"], g["ua_flag"]) for g, _ in done}
    assert len(flags) >= 12, flags
    assert {g["transport_id"] >= 0 for g, _ in done if g["ua_flag"]} == {True, False}
    for cut in (1, 7, 10 ** 6):
        lib_side = dab.PacketGroups()
        got = _groups_through(lib_side, recs, data, cut)
        _assert_groups_equal(got, done, cut)
        assert list(lib_side.stats()) == model.stat_list()
        lib_side.close()


def _pk(cell, addr, ci, fl, useful, cmd=0):
    return (cell, addr, 1, ci, fl, cmd, len(useful), 0), np.frombuffer(bytes(useful), dtype=np.uint8)


def test_data_group_rule_every_drop():
    rng = np.random.default_rng(22)
    g = m.make_group(rng, 40, crc=1)
    broken = g.copy()
    broken[10] ^= 4
    seq = [
        _pk(0, 9, 0, 0, b"orphan intermediate"), _pk(1, 9, 1, 1, b"orphan last"),                    # no open group
        _pk(2, 9, 0, 2, g[:19]), _pk(3, 9, 1, 0, g[19:30]), _pk(4, 9, 2, 1, g[30:]),                    # a group in three packets
        _pk(5, 9, 3, 2, b"unfinished"), _pk(6, 9, 0, 2, broken[:19]), _pk(7, 9, 1, 1, broken[19:]),    # dropped by the next first; then a CRC fail
        _pk(8, 9, 2, 2, b"continuity"), _pk(9, 9, 0, 1, b"skips"),                                     # 2 -> 0: dropped
        _pk(10, 9, 1, 1, b"after the drop"),                                                           # orphan
        _pk(11, 0, 0, 3, b"padding"), _pk(12, 9, 0, 3, b"command", cmd=1),                             # passed over
        _pk(13, 9, 3, 3, g), _pk(14, 12, 0, 2, g[:7]), _pk(15, 9, 0, 3, b"x"), _pk(16, 12, 1, 1, g[7:]),  # one and only; two addresses interleaved
    ]
    seq.append(_pk(17, 30, 0, 2, bytes(19)))
    ci = 0
    for i in range(8208 // 19 - 1):                               # 19 + 431 x 19 = 8208 bytes exactly, then one byte more
        ci = (ci + 1) % 4
        seq.append(_pk(18 + i, 30, ci, 0, bytes(19)))
    seq.append(_pk(500, 30, (ci + 1) % 4, 1, b"z"))
    seq.append(_pk(501, 30, (ci + 2) % 4, 1, b"orphan again"))
    recs, data = [r for r, _ in seq], [d for _, d in seq]
    model = m.Groups()
    done = model.push(recs, data)
    assert [(x["address"], x["length"], x["crc_flag"], x["crc_ok"]) for x, _ in done] == [(9, 40, 1, 1), (9, 40, 1, 0), (9, 40, 1, 1), (9, 1, 0, 0), (12, 40, 1, 1)]
    assert model.stats == dict(groups=5, dropped=3, orphan_packets=4, crc_fails=1), model.stats
    assert done[3][0]["header_ok"] == 0
    for cut in (1, 4, 10 ** 6):
        lib_side = dab.PacketGroups()
        _assert_groups_equal(_groups_through(lib_side, recs, data, cut), done, cut)
        assert list(lib_side.stats()) == model.stat_list()
        lib_side.close()


def test_every_flag_combination():
    rng = np.random.default_rng(23)
    recs, data, n = [], [], 0
    for bits in range(32):
        ext, crc, seg, ua, tid = (bits >> 4) & 1, (bits >> 3) & 1, (bits >> 2) & 1, (bits >> 1) & 1, bits & 1
        g = m.make_group(rng, 30, gtype=bits & 15, ext=ext, crc=crc, seg=seg, ua=ua, tid=tid, ci=bits & 15, rep=(bits >> 1) & 15)
        r, d = _pk(n, 100 + bits, 0, 3, g)
        recs.append(r)
        data.append(d)
        n += 1
    for cut_to in (1, 2, 3, 4, 5, 6):                             # groups too short for the header their flags announce
        r, d = _pk(n, 200 + cut_to, 0, 3, bytes([0xB0 | 1, 0, 1, 2, 0x12, 9][:cut_to]))
        recs.append(r)
        data.append(d)
        n += 1
    model = m.Groups()
    done = model.push(recs, data)
    assert len(done) == 38
    for bits, (g, _) in enumerate(done[:32]):
        assert (g["ext_flag"], g["crc_flag"], g["seg_flag"], g["ua_flag"]) == ((bits >> 4) & 1, (bits >> 3) & 1, (bits >> 2) & 1, (bits >> 1) & 1)
        assert g["header_ok"] and g["crc_ok"] == g["crc_flag"] and (g["segment_number"] >= 0) == bool(g["seg_flag"])
        assert (g["transport_id"] >= 0) == bool(g["ua_flag"] and bits & 1)
    assert [g["header_ok"] for g, _ in done[32:]] == [0, 0, 0, 0, 0, 0]
    lib_side = dab.PacketGroups()
    _assert_groups_equal(_groups_through(lib_side, recs, data, 5), done, "flags")
    lib_side.close()


def test_library_and_binding_know_the_stage():
    for name in ("dabhip_packet_create", "dabhip_packet_push", "dabhip_packet_records", "dabhip_packet_data", "dabhip_packet_stats", "dabhip_packet_stage_ms",
                 "dabhip_packet_groups_push"):
        assert name in dab.exported_symbols()
    if dab.lib().dabhip_device_count() == 0:
        with pytest.raises(dab.DabhipError, match="no HIP device"):
            dab.Packet(1, [3], [1])


def test_host_rule_under_sanitizers():
    here = os.path.join(ROOT, "tests", "host_sanitize")
    os.makedirs(os.path.join(here, "build"), exist_ok=True)
    exe = os.path.join(here, "build", "packet_units_asan")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(here, "packet_units.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "Sanitizer" not in run.stderr, run.stderr[-4000:]
    out = run.stdout.split("\n")
    assert out[0].split() == ["ok", "packet-units"]
    # the fullest slot array of the property: the most a push of 64 frames can give, floor((102 + 64 x 255) / 103), in the 162 slots planned for it
    assert out[1].startswith("fullest 159 of 162 slots: 255 cells per frame,") and out[1].endswith("64 frames"), out[1]


# ---- the modulator's packet-mode content ----------------------------------------------------------------------------------------------------------
def _packet_cfg(seed, phase=0, fec_mask=0b0101):
    """Preset 1 with every slot a packet-mode slot; FEC on the slots of fec_mask."""
    cfg = dab.synth_preset(1, seed=seed)
    cfg.packet_slots = (1 << cfg.nsub) - 1
    cfg.packet_fec_slots = fec_mask & cfg.packet_slots
    cfg.packet_phase = phase
    return cfg


def test_modulator_is_off_by_default_and_leaves_the_other_slots_alone():
    plain = dab.synth_preset(1, seed=9)
    assert plain.packet_slots == 0 and plain.packet_fec_slots == 0 and plain.packet_phase == 0
    cfg = dab.synth_preset(1, seed=9)
    cfg.packet_slots = cfg.packet_fec_slots = 1 << 2
    for cif in (0, 7, 300):
        assert (dab.synth_fibs(cfg, cif) == dab.synth_fibs(plain, cif)).all()
        for slot in range(plain.nsub):
            same = (dab.synth_payload(cfg, cif, slot) == dab.synth_payload(plain, cif, slot)).all()
            assert same == (slot != 2), (cif, slot)
    assert (dab.synth_generate(dab.synth_preset(1, seed=9), 2) == dab.synth_generate(plain, 2)).all()


def test_modulator_cells_and_groups_against_the_model():
    for phase in (0, 40, 102):
        cfg = _packet_cfg(77 + phase, phase)
        for slot in range(cfg.nsub):
            s = dab.synth_payload(cfg, 0, slot).size // 24
            fec = bool(cfg.packet_fec_slots >> slot & 1)
            addresses = dab.synth_packet_addresses(cfg, slot)
            assert len(addresses) in (2, 3) and len(set(addresses)) == len(addresses) and all(0 < a < 1022 for a in addresses)
            seen = {a: 0 for a in addresses}
            kinds, lengths, flags = set(), set(), set()
            for j in range(6 if fec else 150):
                if fec:
                    cells = dab.synth_packet_cells(cfg, slot, 103 * j + phase, 103)
                    assert (m.fec_frame(cells[:94].reshape(-1)) == cells.reshape(-1)).all(), (phase, slot, j)
                    unit = cells[:94]
                else:
                    unit = dab.synth_packet_cells(cfg, slot, s * j, s)
                recs, groups = cs.unit_groups(unit)
                for r in recs:
                    kinds.add("padding" if r[1] == 0 else "command" if r[5] else "data")
                    lengths.add(r[2])
                    assert r[1] == 0 or r[1] in addresses
                for a, g in groups:                               # the n-th group of an address, counted from unit 0
                    assert (dab.synth_packet_group(cfg, slot, a, seen[a]) == g).all(), (phase, slot, j, a, seen[a])
                    seen[a] += 1
                    flags.add(int(g[0]) >> 4)
            assert kinds == {"padding", "command", "data"} and (lengths == {1, 2, 3, 4} or s < 4), (slot, kinds, lengths)
            assert min(seen.values()) > 0 and (len(flags) >= 8 or not fec), (slot, seen, flags)
            # what the CIFs carry is those cells; a frame before frame 0 fills the cells in front of packet_phase
            stream = np.concatenate([dab.synth_payload(cfg, cif, slot) for cif in range(3)])
            assert (stream == dab.synth_packet_cells(cfg, slot, 0, 3 * s).reshape(-1)).all()
            if fec and phase:
                before = dab.synth_packet_cells(cfg, slot, phase - 103, 103)
                assert (m.fec_frame(before[:94].reshape(-1)) == before.reshape(-1)).all()
                n = min(phase, 3 * s)
                assert (before[103 - phase:][:n].reshape(-1) == stream[:24 * n]).all()


def test_modulator_refusals():
    def refused(change, call=lambda c: dab.synth_payload(c, 0, 0)):
        cfg = _packet_cfg(5)
        change(cfg)
        with pytest.raises(dab.DabhipError):
            call(cfg)

    def past_nsub(c):
        c.packet_slots |= 1 << c.nsub

    def also_dabplus(c):
        c.dabplus_slots = 1

    def fec_only(c):
        c.packet_slots &= ~1

    # (every bit rate a valid multiplex can give is a multiple of 8 kbit/s: that refusal cannot be reached from here)
    refused(past_nsub)
    refused(also_dabplus)
    refused(fec_only)
    refused(lambda c: c.set_reconf(0, 40, c.multiplex()))
    refused(lambda c: None, lambda c: dab.synth_packet_cells(dab.synth_preset(1, seed=5), 0, 0, 1))     # not a packet-mode slot
    refused(lambda c: None, lambda c: dab.synth_packet_group(c, 0, 1023, 0))                            # no such group
    dab.synth_payload(_packet_cfg(5), 0, 0)
