"""The EDI receiving model (tests/edirx_model.py) and the stage's host-only parts on the CPU: known answers that need no second implementation
(any 48 erased bytes of a word from the sender's encoder come back, 49 cannot be asked for, a damaged word is seen), receive(pack(frames)) ==
rebuild(carried(frame)) on the crafted frames in all three modes, m_max >= recover on the whole grid of the size rule, the window rule under
every cutting into pushes and by hand, and tests/host_sanitize/edirx_units.cpp, a stand-alone program, under ASan + UBSan: the packet checks,
the window rule, the TAG walk and the rebuild of csrc/edirx_plan.hpp against vectors the model wrote, truncated and lying length fields
among them."""
import os
import struct
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import edi_cases as ecs
import edi_model as em
import edirx_cases as cs
import edirx_model as rx
import eti_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- known answers ---------------------------------------------------------------------------------------------------------------------------------
def test_any_48_erased_bytes_come_back_and_49_cannot_be_asked_for():
    rng = np.random.default_rng(48)
    for k in (1, 57, 204, 207):
        data = rng.integers(0, 256, (1, k), dtype=np.uint8)
        word = np.zeros(255, np.uint8)
        word[:k] = data[0]
        word[207:] = em.rs_parity(data)[0]
        assert not rx.syndromes(word).any()
        live = np.concatenate([np.arange(k), np.arange(207, 255)])
        for n in (1, 2, 47, 48):
            places = sorted(rng.choice(live, min(n, live.size), replace=False).tolist())
            broken = word.copy()
            broken[places] = rng.integers(0, 256, len(places), dtype=np.uint8)
            assert (rx.fill_erasures(broken, places) == word).all(), (k, n)
        places = sorted(rng.choice(live, min(40, live.size - 1), replace=False).tolist())
        other = [int(j) for j in live if j not in places][0]
        broken = word.copy()
        broken[other] ^= 0x40                          # an error beside the erasures
        assert rx.fill_erasures(broken, places) is None, k
    with pytest.raises(ValueError):
        rx.fill_erasures(np.zeros(255, np.uint8), list(range(49)))


def test_crc_check_value_and_field_tables():
    assert rx.crc(b"123456789") == 0xD64E
    assert sorted(rx.ALOG.tolist()) == list(range(1, 256)) and rx.ALOG[8] == 0x1D


def test_m_max_is_never_below_recover_on_the_grid_and_its_fragments_fit_48_bytes():
    seen = set()
    for l in ecs.GRID_L:
        for recover in ecs.GRID_RECOVER:
            for F in ecs.GRID_FRAG:
                c, k, z, B, f, s = em.plan(l, 2, recover, F)
                key = (c, k, f)
                if key in seen:
                    continue
                seen.add(key)
                mm = rx.m_max(k, f)
                assert recover <= mm < f, (l, recover, F)
                # the worst mm fragments of the worst word
                worst = max(len(rx.word_erasures(set(range(f)) - set(range(a, a + mm)), f, k, w)) for w in (0, c - 1) for a in (0, f - mm)) if mm else 0
                assert worst <= 48, (l, recover, F)


def test_the_two_shapes_at_the_edge_of_48():
    assert em.plan(204, 2, 5, 1400) == (1, 204, 0, 252, 32, 8) and rx.m_max(204, 32) == 6
    assert cs.erasure_counts(204, 5, 1400, range(6)) == [48] and cs.erasure_counts(204, 5, 1400, [0, 1, 2, 3, 4, 31]) == [47]
    assert em.plan(6620, 2, 5, 64) == (32, 207, 4, 8160, 128, 64) and rx.m_max(207, 128) == 24
    counts = cs.erasure_counts(6620, 5, 64, [127])
    assert set(counts) == {1, 2} and cs.erasure_counts(6620, 5, 64, range(24)) .count(48) >= 1


# ---- receive(pack(frames)) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,recover,max_frag", cs.MODES + [(2, 5, 64)])
def test_receive_of_pack_gives_the_rebuilt_frames(mode, recover, max_frag):
    frames = ecs.border_frames()
    want = cs.expected_frames(frames)
    groups = cs.packets_of(frames, mode, recover, max_frag, 65534)
    got, recs, stats = rx.receive(cs.flat(groups))
    assert len(got) == len(want) == len(frames) - 4
    assert all((a == b).all() for a, b in zip(got, want))
    assert [r[1] for r in recs] == [(65534 + i) & 0xFFFF for i in range(len(want))] and [r[0] for r in recs] == list(range(len(want)))
    assert stats == [sum(len(g) for g in groups)] + [0] * 13 + [len(want)]
    if mode == 2:                                       # the most fragments the sender promised to survive, first ones and last ones
        lossy = cs.flat([cs.drop(g, range(recover)) if i % 2 else cs.drop(g, range(len(g) - recover, len(g))) for i, g in enumerate(groups)])
        got, recs, stats = rx.receive(lossy)
        assert len(got) == len(want) and all((a == b).all() for a, b in zip(got, want))
        assert all(r[4] == r[5] - recover and (r[6] > 0) == (recover > 0) for r in recs) and stats[rx.STATS.index("words_filled")] == sum(r[6] for r in recs)


def test_a_rebuilt_frame_is_a_fixed_point_and_passes_the_eti_checker():
    """rebuild(carried(F)) == F once F has what the engine writes (FL in bytes 6..7, both CRCs, the FF bytes, 0x55 padding); with the engine's
    STAT and MNSC (FF) tests/eti_check.py accepts it"""
    rng = np.random.default_rng(4)
    d = em.carried(ecs.frame(rng, 7, [3, 0, 5]))
    f = rx.rebuild(d)
    assert (rx.rebuild(em.carried(f)) == f).all()
    d.update(err=0xFF, mnsc=0xFFFF)
    parsed = eti_check.parse(rx.rebuild(d))
    assert parsed["nst"] == 3 and parsed["fct"] == 7 and [s[3] for s in parsed["stc"]] == [3, 0, 5]


# ---- the window ------------------------------------------------------------------------------------------------------------------------------------
def _collect(r, pushes, flush=True):
    out = []
    for p in pushes:
        out += r.push(p)
    if flush:
        out += r.flush()
    return [x[0].tobytes() for x in out], [x[1] for x in out], r.stat_list()


def test_window_rule_under_every_cutting_into_pushes():
    frames = cs.small_stream(4, 3)
    g = cs.packets_of(frames, 2, 0, 64, 65534)                               # 2, 5, 4, 4 fragments; m_max 1
    lossy = cs.drop(g[1], [1])
    packets = g[0][:1] + lossy[:2] + g[0][1:] + lossy[2:] + g[2]                          # out of order within the window, one group short of a fragment
    whole = _collect(rx.Receiver(2), [packets])
    assert len(packets) == 10 and whole[2][rx.STATS.index("frames")] == 3 and whole[2][rx.STATS.index("words_filled")] >= 1
    for sizes in ecs.cuttings(len(packets)):
        assert _collect(rx.Receiver(2), cs.cut(packets, [0] + sizes + [0])) == whole, sizes


def test_window_by_hand():
    frames = cs.small_stream(8, 5)
    af = [g[0] for g in cs.packets_of(frames, 0, seq0=65534)]                # SEQ 65534, 65535, 0, 1, ..
    want = [f.tobytes() for f in cs.expected_frames(frames)]
    got, recs, stats = _collect(rx.Receiver(4), [af])
    assert got == want and [r[1] for r in recs] == [65534, 65535, 0, 1, 2, 3, 4, 5]
    # swapped pairwise: the same frames in the same order
    swapped = [af[0]] + [af[1 + (i ^ 1)] for i in range(6)] + [af[7]]       # behind the first packet, which sets the window
    assert _collect(rx.Receiver(4), [swapped])[0] == want
    # depth 1: the packet that comes early pushes the window on; the one it overtook is late
    got, recs, stats = _collect(rx.Receiver(1), [swapped])
    assert got == [want[i] for i in (0, 2, 4, 6, 7)] and stats[rx.STATS.index("late")] == 3 and stats[rx.STATS.index("missing")] == 3
    # a jump of 20,000: every number between counts as missing
    jump = cs.packets_of(frames[:2], 0, seq0=20005)
    got, recs, stats = _collect(rx.Receiver(4), [af[:3] + cs.flat(jump)])
    # next is 1; 20005 takes the window to 20002 .. 20005 (1 .. 20001 missing), 20006 to 20003 .. 20006 (20002 missing); the flush counts none
    assert len(got) == 5 and stats[rx.STATS.index("missing")] == 20002 and [r[1] for r in recs][-2:] == [20005, 20006]
    # duplicates, and a second AF packet that differs only in kind
    g = cs.packets_of(frames[1:2], 1, 0, 64, 9)[0]
    got, recs, stats = _collect(rx.Receiver(4), [[g[0], g[0]] + [cs.make_af(frames[1], 9)] + g[1:]])
    assert len(g) > 1 and got == want[1:2] and stats[rx.STATS.index("duplicates")] == 1 and stats[rx.STATS.index("mismatched")] == 1
    # reset: the window forgets, the numbers go on
    r = rx.Receiver(4)
    r.push(af[:2])
    r.reset()
    out = r.push(af[:2])
    assert [x[1][0] for x in out] == [2, 3] and r.stats["late"] == 0


def test_foreign_items_time_stamp_and_rfud():
    rng = np.random.default_rng(11)
    f = ecs.frame(rng, 9, [4, 2])
    want = rx.rebuild(em.carried(f)).tobytes()
    plain = cs.make_af(f, 0)
    assert plain == em.af_body(f, 0, 0) + em.crc16(em.af_body(f, 0, 0)).to_bytes(2, "big")
    cases = [cs.make_af(f, 0, between=[(b"*dmy", bytes(5)), (b"avtm", b"xyz")]), cs.make_af(f, 1, atst=bytes(range(8))), cs.make_af(f, 2, rfud=b"\x01\x02\x03"),
             cs.make_af(f, 3, ptr=False)]
    got, recs, stats = _collect(rx.Receiver(4), [cases])
    assert got == [want] * 4 and stats[rx.STATS.index("items_ignored")] == 2 and stats[rx.STATS.index("with_atst")] == 1
    bad = [cs.make_af(f, 0, between=[(b"est\x07", bytes(3))]), cs.make_af(f, 1, atst=bytes(7)), cs.make_af(f, 2, between=[(b"*ptr", b"DETJ" + bytes(4))])]
    got, recs, stats = _collect(rx.Receiver(4), [bad])
    assert got == [] and stats[rx.STATS.index("groups_refused")] == 3


# ---- the binding -----------------------------------------------------------------------------------------------------------------------------------
def test_binding_exports_the_stage():
    names = {"dabhip_edirx_" + n for n in ("create", "destroy", "push", "flush", "records", "frames", "reset", "stats", "stage_ms")}
    assert names <= set(dab.exported_symbols())
    assert dab.EDIRX_STATS == rx.STATS and dab.EDIRX_REC.itemsize == 32 and len(dab.EDIRX_STAGES) == 7 and callable(dab.EdiRx.flush)
    if dab.lib().dabhip_device_count() == 0:
        with pytest.raises(dab.DabhipError, match="no HIP device"):
            dab.EdiRx(1)


# ---- the shared header under sanitizers ------------------------------------------------------------------------------------------------------------
def _units_exe():
    here = os.path.join(ROOT, "tests", "host_sanitize")
    os.makedirs(os.path.join(here, "build"), exist_ok=True)
    exe = os.path.join(here, "build", "edirx_units_asan")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(here, "edirx_units.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    return exe


def _run_units(args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "Sanitizer" not in run.stderr, run.stderr[-4000:]
    out = run.stdout.split("\n")
    assert out[0].split() == ["ok", "edirx-units"]
    return out[1].split()


def _write_items(path, items):
    with open(path, "wb") as fp:
        fp.write(struct.pack("<I", len(items)))
        for x in items:
            fp.write(struct.pack("<I", len(x)) + bytes(x))


def _lying_packets():
    """good packets of every kind, every truncation of one of each down to nothing, and length fields that lie"""
    frames = cs.small_stream(3, 8)
    af = cs.packets_of(frames, 0)[0][0]
    pf = cs.packets_of(frames, 1, 0, 64)[1][1]
    fec = cs.packets_of(frames, 2, 3, 64)[1][2]
    out = [af, pf, fec]
    for p in (af, pf, fec):
        out += [p[:n] for n in range(0, 20)] + [p[:-1], p + b"\x00"]
    out += [cs.rehead(pf, plen=len(pf) - 13), cs.rehead(pf, plen=0x3FFF), cs.rehead(fec, findex=fec[9]), cs.rehead(fec, fcount=257, findex=0), cs.rehead(fec, rsk=0),
            cs.rehead(fec, rsk=208), cs.rehead(fec, rsz=200), cs.with_byte_flipped(pf, 13), cs.with_byte_flipped(af, 8, 0x80), b"PF" + bytes(10), b"AF" + b"\xff" * 10,
            af[:2] + (len(af) - 11).to_bytes(4, "big") + af[6:]]
    return out


def test_rule_header_under_sanitizers(tmp_path):
    exe = _units_exe()
    # 1. the packet checks
    packets = _lying_packets()
    _write_items(tmp_path / "p.bin", packets)
    words = _run_units([exe, "check", str(tmp_path / "p.bin")])
    kinds = {"AF": 1, "PF": 2, "FEC": 3}
    want = []
    for p in packets:
        h = rx.check_packet(p)
        want.append("0:0" if h is None else "%d:%d" % (kinds[h["kind"]], rx.m_max(h["rsk"], h["fcount"]) if h["kind"] == "FEC" else 0))
    assert words == ["kinds:"] + want and want[:3] == ["1:0", "2:0", want[2]] and want[2].startswith("3:") and want.count("0:0") >= 60
    # 2. the walk and the rebuild: good packets, foreign items, and lengths that lie inside a right LEN
    rng = np.random.default_rng(2)
    f = ecs.frame(rng, 3, [2, 0, 6])
    afs = [g[0] for g in cs.packets_of(ecs.border_frames(), 0)]
    afs += [cs.make_af(f, 0, between=[(b"*dmy", bytes(5))]), cs.make_af(f, 0, atst=bytes(8), rfud=bytes(3)), cs.make_af(f, 0, atst=bytes(7)), cs.make_af(f, 0, ptr=False)]
    base = cs.make_af(f, 0)
    for at in (14, 15, 16, 17, 30, 31, 32, 33, 34, 35):                      # the length fields of *ptr and deti, and deti's flags
        afs.append(cs.with_byte_flipped(base, at, 0xFF))
        afs.append(cs.with_byte_flipped(base, at, 0x01))
    afs += [base[:12 + n] for n in (0, 7, 8, 9, 16, 24, 30, 38)]             # cut anywhere (LEN is the caller's business here)
    _write_items(tmp_path / "a.bin", afs)
    words = _run_units([exe, "walk", str(tmp_path / "a.bin"), str(tmp_path / "a.eti")])
    fields = [rx.walk(a) for a in afs]
    assert [w != "0" for w in words[1:]] == [d is None for d in fields] and sum(d is None for d in fields) >= 10
    assert (tmp_path / "a.eti").read_bytes() == b"".join(rx.rebuild(d).tobytes() for d in fields if d is not None)
    # 3. streams through the window: every mode whole, out of order, with loss, duplicates, bad packets, a jump and the wrap of SEQ
    frames = ecs.border_frames()[:12] + cs.small_stream(6, 9)
    streams = {}
    for mode, recover, max_frag in cs.MODES:
        streams["mode%d" % mode] = (4, cs.flat(cs.packets_of(frames, mode, recover, max_frag, 65530)))
    g = cs.packets_of(frames, 1, 0, 255, 65530)
    rnd = np.random.default_rng(6)
    shuffled = []
    for a in range(0, len(g), 3):
        part = cs.flat(g[a:a + 3])
        shuffled += [part[i] for i in rnd.permutation(len(part))]
    streams["shuffled"] = (3, shuffled)
    lossy = cs.flat([cs.drop(x, [0]) if i % 3 == 0 else x for i, x in enumerate(cs.packets_of(frames, 2, 1, 64, 7))])
    streams["lossy"] = (2, lossy[:40] + [lossy[3], b"junk", cs.rehead(lossy[41], rsk=7)] + lossy[40:])
    streams["jump"] = (16, cs.flat(cs.packets_of(frames[:3], 0, seq0=5)) + cs.flat(cs.packets_of(frames[3:6], 1, 0, 64, 30005)))
    for name, (depth, packets) in streams.items():
        _write_items(tmp_path / "s.bin", packets)
        got, recs, stats = rx.receive(packets, depth)
        with_rs = sum(1 for r in recs if r[6] > 0)
        plain = [fr.tobytes() for fr, r in zip(got, recs) if r[6] == 0]
        for cuts in (0, 1):
            words = _run_units([exe, "stream", str(tmp_path / "s.bin"), str(depth), str(cuts), str(tmp_path / "s.eti")])
            cnt = [int(v) for v in words[1:16]]
            want = list(stats)
            for key in ("words_filled", "erasures_filled"):
                want[rx.STATS.index(key)] = 0
            want[rx.STATS.index("frames")] -= with_rs
            assert cnt == want and int(words[17]) == with_rs, (name, cuts, cnt, want, words)
            assert (tmp_path / "s.eti").read_bytes() == b"".join(plain), name
