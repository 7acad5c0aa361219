"""The ensemble directory without a GPU: the plain model (tests/dir_model.py) against the project's reference-pinned FIC parse on well-formed FIBs,
against hand-written vectors rule by rule, against the rule header dir_figs.hpp (tests/host_sanitize/dir_units.cpp, a stand-alone program under
ASan + UBSan), and the modulator's si_mode against the model.  eti2info builds its directory on the GPU like eti2ts, so its test is in
test_gpu_dir.py."""
import os
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import dir_cases as cs
import dir_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the model against the parse that is held to the reference (fic.c) -----------------------------------------------------------------------
def _well_formed_groups(rng, ngroups):
    """groups of 12 FIBs holding only FIG 0/0, 0/1 (both forms) and 0/2 (TMId 0..3, P/D 0 and 1), C/N = OE = 0, exact lengths; every UEP index
    and every EEP level occurs"""
    uep, eep = 0, 0
    groups = []
    for _ in range(ngroups):
        ids = [int(x) for x in rng.permutation(64)]                  # every SubChId at most once per group in FIG 0/1
        fibs = []
        for _ in range(12):
            figs, room = [], 30
            while True:
                what = int(rng.integers(0, 3))
                if what == 0:
                    f = cs.fig0(0, cs.e00(int(rng.integers(0, 65536)), cif_hi=int(rng.integers(0, 20)), cif_lo=int(rng.integers(0, 250))))
                elif what == 1:
                    body = b""
                    for _ in range(int(rng.integers(1, 5))):
                        if not ids:
                            break
                        if rng.random() < 0.5:
                            body += cs.e01_short(ids.pop(), int(rng.integers(0, 864)), uep % 64)
                            uep += 1
                        else:
                            option, level = (eep // 4) % 2, eep % 4
                            eep += 1
                            body += cs.e01_long(ids.pop(), int(rng.integers(0, 864)), option, level, M.EEP_MULTIPLE[option * 4 + level] * int(rng.integers(1, 9)))
                    f = cs.fig0(1, body)
                else:
                    pd = int(rng.integers(0, 2))
                    comps = []
                    for _ in range(int(rng.integers(0, 4))):
                        tmid = int(rng.integers(0, 4))
                        comps.append(cs.comp(tmid, int(rng.integers(0, 64)), int(rng.integers(0, 64))) if tmid < 2 else cs.comp(tmid, int(rng.integers(0, 4096))))
                    f = cs.fig0(2, cs.e02(int(rng.integers(0, 1 << (32 if pd else 16))), comps, pd=pd), pd=pd)
                if len(f) > room:
                    break
                figs.append(f)
                room -= len(f)
            fibs.append(cs.fib(*figs))
        groups.append(fibs)
    assert uep >= 64 and eep >= 8
    return groups


def test_model_against_the_reference_pinned_parse():
    rng = np.random.default_rng(11)
    groups = _well_formed_groups(rng, 170)
    assert 12 * len(groups) >= 2000
    seen_uep, seen_eep = set(), set()
    for fibs in groups:
        hdr, sub = dab.host_parse_fibs(np.frombuffer(b"".join(fibs), dtype=np.uint8), np.ones(12, dtype=np.uint8))
        m = M.Stream()
        ascty = {}
        for k in range(4):
            m.push(cs.frame(fibs[3 * k:3 * k + 3]))
        for f in fibs:
            facts, _, trunc, ign = M.walk_fib(f)
            assert trunc == 0 and ign == 0
            for kind, _, fields in facts:
                if kind == "0/2":
                    for c0, c1 in zip(fields[1][0::2], fields[1][1::2]):
                        if c0 >> 6 == 0:
                            ascty[c1 >> 2] = c0 & 63
        assert m.c["figs_truncated"] == 0 and m.c["figs_ignored"] == 0 and m.c["fibs_crc_failed"] == 0
        if m.ens is not None:
            eid, _, _, hi, lo = m.ens.parts["0/0"]
            assert (eid, hi, lo) == tuple(int(x) for x in hdr)
        else:
            assert tuple(hdr) == (0, 0, 0)
        for i in range(64):
            row = [int(x) for x in sub[i]]
            if i in m.sub:
                form, index, protlev, start, size, rate = m.sub[i].parts["0/1"]
                assert row[0] == i and row[1] == form and row[3:7] == [start, size, rate, protlev], (i, row, m.sub[i].parts)
                if not form:
                    assert row[2] == index
                    seen_uep.add(index)
                else:
                    seen_eep.add(protlev)
            else:
                assert row[0] == -1
            assert row[7] == ascty.get(i, -1)
    assert seen_uep == set(range(64)) and seen_eep == set(range(8))


# ---- 2. hand-written vectors, one per rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cs.VECTORS))
def test_walk_rule(name):
    fib, facts, counts = cs.VECTORS[name]
    assert M.fib_crc_ok(fib)
    got = M.walk_fib(fib)
    assert got[0] == facts
    assert got[1:] == counts


def test_frame_rules_and_crc():
    good = cs.fib(cs.fig0(14, cs.e14(5, 1)))
    m = M.Stream()
    assert m.push(cs.frames([[good]], nst=0)) == 3
    assert m.push(cs.frames([[good]], nst=64)) == 3
    assert m.push(cs.frames([[good]], nst=65)) == 0
    assert m.push(cs.frames([[good]], mid=2)) == 0
    assert m.push(cs.frames([[good]], ficf=0)) == 0
    assert m.push(cs.frames([[good]], ficf=0, mid=3, nst=100)) == 0               # FICF is looked at first
    assert m.push(cs.frames([[cs.fib(cs.fig0(14, cs.e14(6, 1)), crc=False), good, cs.fib(crc=False)]])) == 1
    assert m.counters() == [7, 2, 2, 9, 2, 3, 0, 0, 3, 0, 0]
    assert m.subch_tuples() == [(5, None, (1,), 0, 6, 0)]
    # the CRC is the one the modulator writes
    cfg = dab.synth_preset(1, seed=2)
    assert all(M.fib_crc_ok(dab.synth_fibs(cfg, 3)[32 * q:32 * q + 32]) for q in range(3))


def test_table_rules():
    lab = lambda ext, sid, text, **kw: cs.fib(cs.label(ext, sid, text, **kw))
    svc = lambda sid, comps, pd=0: cs.fib(cs.fig0(2, cs.e02(sid, comps, pd=pd), pd=pd))
    three = [cs.comp(0, 63, 1), cs.comp(1, 24, 2, ps=0), cs.comp(3, 9, ps=0)]
    m = M.Stream()
    m.push(cs.frames([
        [lab(1, 0x1111, "before its 0/2"), svc(0x2222, three), svc(0x2222, three)],                  # frame 0: a label first; equal bytes twice
        [svc(0x1111, three[:1]), lab(1, 0x2222, "after its 0/2"), svc(0xE0001111, three[2:], pd=1)],  # frame 1: P/D 1 with the same low 16 bits
        [svc(0x2222, three[:1]), lab(1, 0x2222, "renamed"), lab(5, 0xE0001111, "data")],             # frame 2: 3 components shrink to 1; a label changes
        [cs.fib(cs.fig0(3, cs.e03(9, 4, 77))), cs.fib(cs.fig0(3, cs.e03(9, 4, 78))), cs.fib(cs.fig0(14, cs.e14(4, 1)))],
        [cs.fib(cs.fig0(1, cs.e01_short(4, 0, 0))), cs.fib(cs.fig0(1, cs.e01_short(4, 0, 0, switch=1))), cs.fib(cs.fig0(1, cs.e01_short(4, 1, 0)))],
        [cs.fib(cs.fig0(0, cs.e00(7)), cs.label(0, 7, "ens")), cs.fib(cs.fig0(10, cs.e10(60000, 1, 2))), cs.fib(cs.fig0(9, cs.e09(1, 2, 3)))],
    ]))
    c0 = (0x3F, 0x06)
    L = lambda t: (0, t.encode().ljust(16), 0xFF00)
    assert m.service_tuples() == [
        ((0, 0x1111), (1, c0), L("before its 0/2"), 0, 1, 0),
        ((0, 0x2222), (1, c0), L("renamed"), 0, 2, 2),
        ((1, 0xE0001111), (1, (0xC0, 0x24)), L("data"), 1, 2, 0)]
    assert m.pkt_tuples() == [(9, (0, 1, 60, 4, 78, 0), 3, 3, 1)]
    assert m.subch_tuples() == [(4, (0, 0, 5, 1, 16, 32), (1,), 3, 4, 1)]              # the table switch is not kept: no change
    assert m.ensemble_tuple() == ((7, 0, 0, 0, 0), (1, 2, 3), (60000, 0, 0, 1, 2, 0, 0), (7, 0, b"ens".ljust(16), 0xFF00), 5, 5, 5, 0)
    assert m.c["facts_changed"] == 4 and m.c["facts"] == 19
    assert not m.complete()                                                           # (0, 0x2222)'s sub-channels 1, 2 have no 0/1
    assert m.resolve(0, 0x2222, 0) == M.NO_SUBCH and m.resolve(0, 0x2222, 1) == M.NO_COMPONENT and m.resolve(0, 0x3333, 0) == M.NO_SERVICE
    assert m.resolve(1, 0xE0001111, 0) == {"kind": "PACKET", "subch": 4, "address": 78, "dg": 1, "dscty": 60, "fec": True, "scid": 9, "primary": 0}
    m.push(cs.frames([[cs.fib(cs.fig0(1, cs.e01_short(1, 100, 5)))]]))
    assert m.complete()
    assert m.resolve(0, 0x1111, 0)["kind"] == "DABPLUS"
    m.push(cs.frames([[svc(0x4444, [cs.comp(3, 10)])]]))
    assert m.resolve(0, 0x4444, 0) == M.NO_PKTCOMP and not m.complete()


def test_table_overflow():
    m = M.Stream()
    frames = [[cs.fib(cs.fig0(2, cs.e02(0x100 + k, []))), cs.fib(cs.fig0(3, cs.e03(k, 1, k))), cs.fib(cs.label(5, 0xE0000000 + k, "x"))] for k in range(33)]
    m.push(cs.frames(frames))
    # 33 services by 0/2 and 33 by label: the 64th is frame 31's label, the 65th and 66th are dropped; 33 SCIds fit
    assert len(m.svc) == 64 and m.svc[63].key == (1, 0xE000001F) and m.c["overflow_dropped"] == 2 and len(m.pkt) == 33
    m.push(cs.frames([[cs.fib(cs.fig0(3, cs.e03(100 + k, 1, k) + cs.e03(200 + k, 1, k)))] for k in range(16)]))
    assert len(m.pkt) == 64 and m.pkt[63].key == 115 and m.c["overflow_dropped"] == 3          # 33 + 31 = 64: SCId 115 is the last, 215 is dropped
    m.push(cs.frames([[cs.fib(cs.fig0(2, cs.e02(0x100, [cs.comp(2, 5)])))]]))               # an existing key in a full table is still updated
    assert m.svc[0].changes == 1 and m.c["overflow_dropped"] == 3


# ---- 3. the rule header under sanitizers ---------------------------------------------------------------------------------------------------------
def _fact_bytes(kind, key, f):
    """a model fact as dir_figs.hpp lays it out: kind, P/D, key (little-endian), payload"""
    be = lambda v, n: int(v).to_bytes(n, "big")
    if kind == "0/0":
        k, pd, sid, p = 1, 0, f[0], be(f[0], 2) + bytes(f[1:])
    elif kind == "0/1":
        k, pd, sid, p = 2, 0, key, bytes(f[:3]) + be(f[3], 2) + be(f[4], 2) + be(f[5], 2)
    elif kind == "0/2":
        k, pd, sid, p = 3, key[0], key[1], (bytes([f[0]]) + bytes(f[1])).ljust(31, b"\0")
    elif kind == "0/3":
        k, pd, sid, p = 4, 0, key, bytes(f[:4]) + be(f[4], 2) + be(f[5], 2)
    elif kind == "0/9":
        k, pd, sid, p = 5, 0, 0, bytes(f)
    elif kind == "0/10":
        k, pd, sid, p = 6, 0, 0, be(f[0], 3) + bytes(f[1:6]) + be(f[6], 2)
    elif kind == "0/14":
        k, pd, sid, p = 7, 0, key, bytes(f)
    elif kind == "ens-label":
        k, pd, sid, p = 8, 0, f[0], be(f[0], 2) + bytes([f[1]]) + f[2] + be(f[3], 2)
    else:
        k, pd, sid, p = 9, key[0], key[1], bytes([f[0]]) + f[1] + be(f[2], 2)
    return bytes([k, pd]) + int(sid).to_bytes(4, "little") + p


def _crc_rows(body):
    """the FIB CRC of n x 30 bytes, all rows at once"""
    crc = np.full(body.shape[0], 0xFFFF, dtype=np.uint32)
    for col in range(30):
        crc ^= body[:, col].astype(np.uint32) << 8
        for _ in range(8):
            crc = np.where(crc & 0x8000, (crc << 1) ^ 0x1021, crc << 1) & 0xFFFF
    return ~crc & 0xFFFF


def test_rule_header_under_sanitizers(tmp_path):
    here = os.path.join(ROOT, "tests", "host_sanitize")
    os.makedirs(os.path.join(here, "build"), exist_ok=True)
    exe = os.path.join(here, "build", "dir_units_asan")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(here, "dir_units.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    rng = np.random.default_rng(21)
    fibs = [fib for fib, _, _ in cs.VECTORS.values()] + [cs.fib(crc=False)] + [cs.hostile_fib(rng) for _ in range(20000)]
    body = rng.integers(0, 256, (100000, 30), dtype=np.uint8)                              # arbitrary bytes under a valid CRC
    crc = _crc_rows(body)
    rows = np.concatenate([body, (crc >> 8).astype(np.uint8)[:, None], (crc & 255).astype(np.uint8)[:, None]], axis=1)
    data = np.concatenate([np.frombuffer(b"".join(fibs), dtype=np.uint8).reshape(-1, 32), rows])
    path = tmp_path / "fibs.bin"
    data.tofile(path)
    h, lines, kinds, ntrunc, nign = 1469598103934665603, [], {}, 0, 0
    for n, fib in enumerate(data, 1):
        ok = M.fib_crc_ok(fib) if n <= len(fibs) else True
        facts, figs, trunc, ign = M.walk_fib(fib) if ok else ([], 0, 0, 0)
        ntrunc += trunc
        nign += ign
        for f in facts:
            kinds[f[0]] = kinds.get(f[0], 0) + 1
        for b in bytes([ok, figs, trunc, ign, len(facts)]) + b"".join(_fact_bytes(*f) for f in facts):
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        if n % 1000 == 0:
            lines.append("%d %016x" % (n, h))
    lines.append("total %d %016x" % (len(data), h))
    # the inputs do reach every entry parser and the walk's edges
    assert len(kinds) == 9 and min(kinds.values()) >= 100 and ntrunc >= 1000 and nign >= 1000, (kinds, ntrunc, nign)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "Sanitizer" not in run.stderr, run.stderr[-4000:]
    got = run.stdout.split("\n")[:-1]
    first_bad = next((i for i, (a, b) in enumerate(zip(got, lines)) if a != b), None)
    assert first_bad is None and len(got) == len(lines), (first_bad, got[first_bad or 0], lines[first_bad or 0])


# ---- 4. the modulator ----------------------------------------------------------------------------------------------------------------------------
def _si_cfg(preset, seed=5):
    cfg = dab.synth_preset(preset, seed=seed)
    cfg.dabplus_slots, cfg.packet_slots, cfg.packet_fec_slots, cfg.ts_slots = 1 << 1, 1 << 2 | 1 << 0, 1 << 2, 1 << 3
    cfg.si_mode = 1
    return cfg


def test_si_mode_off_leaves_the_fibs_alone():
    """si_mode = 0: the FIBs are FIG 0/0 and FIG 0/1 alone, byte for byte what the model of the packing before si_mode gives"""
    for preset in (0, 1):
        cfg = dab.synth_preset(preset, seed=4)
        cfg.dabplus_slots = 1 << 1
        assert cfg.si_mode == 0
        for cif in range(100):
            fibs = dab.synth_fibs(cfg, cif)
            count = cif % 5000
            figs = [bytes([0x05, 0x00, cfg.eid >> 8, cfg.eid & 255, count // 250, count % 250])]
            entries = [cs.e01_long(s.id, s.start_cu, s.eep_protlev >> 2, s.eep_protlev & 3, s.size_cu) if s.slform else cs.e01_short(s.id, s.start_cu, s.uep_index)
                       for s in cfg.sub[:cfg.nsub]]
            want, nxt = [], 0
            for f in range(3):
                body = figs[0] if f == 0 else b""
                take = b""
                while nxt < len(entries) and len(body) + 2 + len(take) + len(entries[nxt]) <= 30:
                    take += entries[nxt]
                    nxt += 1
                if take:
                    body += bytes([1 + len(take), 0x01]) + take
                body = (body + b"\xff").ljust(30, b"\0")[:30]
                c = ~M.crc16(body) & 0xFFFF
                want.append(body + bytes([c >> 8, c & 255]))
            assert bytes(fibs) == b"".join(want), (preset, cif)


def test_si_mode_names_every_slot():
    for preset in (0, 1):
        cfg = _si_cfg(preset)
        m = M.Stream()
        for cif in range(200):
            f = bytes(dab.synth_fibs(cfg, cif))
            m.push(cs.frame([f[0:32], f[32:64], f[64:96]]))
        assert m.complete() and m.c["figs_truncated"] == 0 and m.c["figs_ignored"] == 0 and m.c["fibs_crc_failed"] == 0
        assert len(m.svc) == cfg.nsub
        for k in range(cfg.nsub):
            kind = "DABPLUS" if cfg.dabplus_slots >> k & 1 else "TS" if cfg.ts_slots >> k & 1 else "PACKET" if cfg.packet_slots >> k & 1 else "MP2"
            pd, sid = (1, 0xE0001000 + k) if kind in ("TS", "PACKET") else (0, 0x1000 + k)
            t = m.resolve(pd, sid, 0)
            assert t["kind"] == kind and t["subch"] == cfg.sub[k].id and t["primary"] == 1, (k, t)
            text = "SLOT %02d %s" % (k, {"DABPLUS": "DAB+"}.get(kind, kind))
            assert next(s for s in m.svc if s.key == (pd, sid)).parts["label"] == (0, text.encode().ljust(16), 0xFF00)
            if kind == "PACKET":
                assert t["address"] == dab.synth_packet_addresses(cfg, k)[0] and t["dg"] == 1 and t["dscty"] == 60 and t["scid"] == k
                assert t["fec"] == bool(cfg.packet_fec_slots >> k & 1)
        ens = m.ens.parts
        assert ens["label"] == (cfg.eid, 0, b"DABHIP SYNTH".ljust(16), 0xFF00) and ens["0/9"] == (0, 0xE1, 1)
        mjd, _, utc, hours, minutes, seconds, ms = ens["0/10"]
        assert (mjd, utc) == (60000, 1) and ((hours * 60 + minutes) * 60 + seconds) * 1000 + ms == 24 * m.ens.time_frame


def test_si_mode_refusals():
    def refused(change):
        cfg = _si_cfg(1)
        change(cfg)
        with pytest.raises(dab.DabhipError):
            dab.synth_fibs(cfg, 0)

    refused(lambda c: c.set_fib_patch(b"\x01\x02"))
    refused(lambda c: c.set_reconf(0, 40, c.multiplex()))
    refused(lambda c: setattr(c, "si_mode", 2))
    dab.synth_fibs(_si_cfg(1), 0)


def test_dir_create_needs_a_gpu_or_says_so():
    try:
        d = dab.Dir(1)
    except dab.DabhipError as e:
        assert "GPU" in str(e) or "HIP" in str(e)
    else:
        d.close()
