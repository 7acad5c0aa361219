"""The ensemble directory on the GPU (dabtools_amd.Dir, k_dir.hip) against the plain model (tests/dir_model.py), field by field and counter by
counter: tables in order, first_frame, last_frame, changes.  Smallest shapes, the walk's and the tables' edges, hostile content, every way of
arrival, and end to end: a modulated capture with service information through the decoder, the directory, and from its plan the DAB+, packet
and TS stages; eti2info on a hand-built ETI file (the tool builds its directory on the GPU, like eti2ts)."""
import json
import os
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import dir_cases as cs
import dir_model as M

pytestmark = pytest.mark.gpu


def _cuts(nframes, chunk, rng):
    """Frame counts of the pushes: fixed, or random with pushes of 0 and 1 frame among them."""
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


def _push(d, streams, chunk=None, how="host", seed=0):
    """Push the streams ((n, 6144) arrays, any lengths) in cuts, the same cut positions for every stream; returns the sum of the pushes' results"""
    rng = np.random.default_rng(seed)
    total, at = 0, 0
    for n in _cuts(max(len(f) for f in streams), chunk, rng):
        parts = [f[at:at + n] for f in streams]
        at += n
        counts = [len(p) for p in parts]
        flat = np.concatenate([np.asarray(p, np.uint8).reshape(-1) for p in parts])
        if how == "host":
            total += d.push(flat, counts)
        else:
            off = 1 if how == "device+1" else 0
            buf = dab.DeviceBuffer(flat.size + 16)
            assert buf.ptr % 16 == 0
            buf.upload(np.concatenate([np.zeros(off, np.uint8), flat, np.zeros(16 - off, np.uint8)]))
            total += d.push((buf.ptr + off, counts))
            buf.free()
    return total


def _models(streams):
    out = []
    for f in streams:
        m = M.Stream()
        m.good = m.push(f)
        out.append(m)
    return out


def _same(d, b, m):
    assert d.stats(b).tolist() == m.counters(), (b, dict(zip(dab.DIR_STATS, d.stats(b))), m.c)
    got, want = cs.gpu_tuples(d, b), cs.model_tuples(m)
    for name, g, w in zip(("ensemble", "sub-channels", "services", "packet components"), got, want):
        assert g == w, (b, name, g, w)
    assert d.complete(b) == m.complete()


def _check(streams, **how):
    d = dab.Dir(len(streams))
    models = _models(streams)
    assert _push(d, streams, **how) == sum(m.good for m in models)
    for b, m in enumerate(models):
        _same(d, b, m)
    d.close()
    return models


def _rich(n, seed):
    """n frames whose FIBs cycle through the hand-written vectors, a carousel of services, labels, packet components and sub-channels that repeat
    with equal and with different bytes, and hostile FIBs"""
    rng = np.random.default_rng(seed)
    vec = [v[0] for _, v in sorted(cs.VECTORS.items())]
    out = []
    for i in range(n):
        k = int(rng.integers(0, 8))
        table = cs.fib(cs.fig0(2, cs.e02(0x1000 + k, [cs.comp(0, 63, k)] * int(rng.integers(0, 2)))), cs.label(1, 0x1000 + k, "SVC %d" % int(rng.integers(0, 2))))
        other = cs.fib(cs.fig0(0, cs.e00(0x4001, cif_lo=i % 250)), cs.fig0(1, cs.e01_short(k, 10 * k, int(rng.integers(0, 2)))),
                       cs.fig0(3, cs.e03(k, k, int(rng.integers(0, 3)))), cs.fig0(14, cs.e14(k, 1)))
        fibs = [vec[(3 * i) % len(vec)], table if i % 2 else cs.hostile_fib(rng), other if i % 3 else vec[(3 * i + 1) % len(vec)]]
        out.append(cs.frame(fibs, nst=int(rng.integers(0, 65)), seed=1000 * seed + i))
    return np.stack(out) if out else np.zeros((0, cs.ETI_BYTES), np.uint8)


# ---- smallest shapes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nframes", [0, 1, 2, 63, 64, 65])
def test_one_stream(nframes):
    (m,) = _check([_rich(nframes, 3)])
    assert m.c["frames"] == nframes and (nframes < 63 or (m.c["facts_changed"] > 0 and m.c["figs_truncated"] > 0 and m.c["figs_ignored"] > 0))


def test_five_streams_of_unequal_length():
    models = _check([_rich(n, 10 + n) for n in (3, 0, 22, 1, 9)])
    assert [m.c["frames"] for m in models] == [3, 0, 22, 1, 9]


@pytest.mark.parametrize("nstreams", [257, 1025])
def test_many_streams(nstreams):
    base = _rich(64, 5)
    streams = [base[(2 * b) % 63:][:2] for b in range(nstreams)]
    streams[-1] = _rich(2, 77)                                        # the last stream is its own
    d = dab.Dir(nstreams)
    models = _models(streams[:32]) + [None] * (nstreams - 33) + _models(streams[-1:])
    want = sum(M.Stream().push(f) for f in streams)
    assert _push(d, streams) == want
    for b in list(range(32)) + [nstreams - 1]:
        _same(d, b, models[b])
    # every stream's counters: equal content gives equal counters
    by_start = {}
    for b in range(nstreams - 1):
        c = d.stats(b).tolist()
        assert by_start.setdefault((2 * b) % 63, c) == c and c[0] == 2, b
    d.close()


def test_frame_headers_and_fic_offsets():
    good = [cs.fib(cs.fig0(14, cs.e14(5, 1))), cs.fib(cs.label(0, 9, "ens")), cs.fib(cs.fig0(0, cs.e00(9)))]
    frames = [cs.frame(good, nst=0, seed=1), cs.frame(good, nst=1, seed=2), cs.frame(good, nst=64, seed=3), cs.frame(good, nst=65, seed=4),
              cs.frame(good, nst=127, seed=5), cs.frame(good, ficf=0, seed=6), cs.frame(good, mid=0, seed=7), cs.frame(good, mid=2, seed=8),
              cs.frame(good, mid=3, seed=9), cs.frame(good, ficf=0, mid=3, nst=100, seed=10)]
    (m,) = _check([np.stack(frames)])
    assert m.counters()[:5] == [10, 2, 5, 9, 0] and m.ens.first == 0 and m.ens.last == 2
    broken = [cs.fib(cs.fig0(14, cs.e14(5, 1)), crc=False)] * 3
    (m,) = _check([np.stack([cs.frame(broken, nst=n) for n in (0, 7, 64)])])
    assert m.counters() == [3, 0, 0, 9, 9, 0, 0, 0, 0, 0, 0] and m.ens is None


# ---- the walk's edges ------------------------------------------------------------------------------------------------------------------------
def test_walk_vectors():
    names = sorted(cs.VECTORS)
    fibs = [cs.VECTORS[n][0] for n in names]
    fibs += [cs.EMPTY_FIB] * (-len(fibs) % 3)
    frames = np.stack([cs.frame(fibs[i:i + 3]) for i in range(0, len(fibs), 3)])
    (m,) = _check([frames])
    want = [sum(cs.VECTORS[n][2][k] for n in names) for k in range(3)]
    assert [m.c["figs"], m.c["figs_truncated"], m.c["figs_ignored"]] == want and m.c["facts"] == sum(len(cs.VECTORS[n][1]) for n in names)
    # one vector per frame, each in a stream of its own: nothing of a FIB leaks into the next
    d = dab.Dir(len(names))
    streams = [np.stack([cs.frame([cs.VECTORS[n][0]], nst=k % 65)]) for k, n in enumerate(names)]
    _push(d, streams)
    for b, n in enumerate(names):
        _, facts, (figs, trunc, ign) = cs.VECTORS[n]
        assert d.stats(b).tolist()[5:9] == [figs, trunc, ign, len(facts)], n
    d.close()


# ---- the tables' edges -----------------------------------------------------------------------------------------------------------------------
def test_table_edges():
    lab = lambda ext, sid, text, **kw: cs.fib(cs.label(ext, sid, text, **kw))
    svc = lambda sid, comps, pd=0: cs.fib(cs.fig0(2, cs.e02(sid, comps, pd=pd), pd=pd))
    three = [cs.comp(0, 63, 1), cs.comp(1, 24, 2, ps=0), cs.comp(3, 9, ps=0)]
    rules = cs.frames([
        [lab(1, 0x1111, "before its 0/2"), svc(0x2222, three), svc(0x2222, three)],
        [svc(0x1111, three[:1]), lab(1, 0x2222, "after its 0/2"), svc(0xE0001111, three[2:], pd=1)],
        [svc(0x2222, three[:1]), lab(1, 0x2222, "renamed"), lab(5, 0xE0001111, "data")],
        [cs.fib(cs.fig0(3, cs.e03(9, 4, 77))), cs.fib(cs.fig0(3, cs.e03(9, 4, 78))), cs.fib(cs.fig0(14, cs.e14(4, 1)))],
        [cs.fib(cs.fig0(1, cs.e01_short(4, 0, 0))), cs.fib(cs.fig0(1, cs.e01_short(4, 0, 0, switch=1))), cs.fib(cs.fig0(1, cs.e01_short(4, 1, 0)))],
        [cs.fib(cs.fig0(0, cs.e00(7)), cs.label(0, 7, "ens")), cs.fib(cs.fig0(10, cs.e10(60000, 1, 2))), cs.fib(cs.fig0(9, cs.e09(1, 2, 3)))],
        [cs.fib(cs.fig0(1, cs.e01_short(1, 100, 5))), cs.fib(cs.fig0(10, cs.e10(60000, 1, 3, seconds=4, ms=5))), cs.fib(cs.fig0(2, cs.e02(1, [cs.comp(0, 0, k) for k in range(12)])))],
    ])
    full = cs.frames([[cs.fib(cs.fig0(2, cs.e02(0x100 + k, []))), cs.fib(cs.fig0(3, cs.e03(k, 1, k))), cs.fib(cs.label(5, 0xE0000000 + k, "x"))] for k in range(33)] +
                     [[cs.fib(cs.fig0(3, cs.e03(100 + k, 1, k) + cs.e03(200 + k, 1, k)))] for k in range(16)] +
                     [[cs.fib(cs.fig0(2, cs.e02(0x100, [cs.comp(2, 5)]))), cs.fib(cs.fig0(3, cs.e03(115, 2, 1))), cs.fib(cs.fig0(3, cs.e03(215, 2, 1)))]])
    a, b = _check([rules, full])
    assert a.c["facts_changed"] == 5 and a.svc[1].changes == 2 and len(a.svc[3].parts["0/2"][1]) == 24 and a.complete() is False
    assert len(b.svc) == 64 and len(b.pkt) == 64 and b.c["overflow_dropped"] == 4 and b.svc[0].changes == 1 and b.pkt[63].changes == 1
    # resolve: every answer and every missing link, against the model
    d = dab.Dir(1)
    d.push(rules)
    codes, kinds = set(), set()
    for pd, sid, ncomp in [(0, 0x1111, 2), (0, 0x2222, 2), (1, 0xE0001111, 2), (0, 1, 13), (0, 0x3333, 1), (1, 0x1111, 1)]:
        for c in range(-1, ncomp):
            want = a.resolve(pd, sid, c)
            if isinstance(want, int):
                with pytest.raises(dab.DirUnresolved) as e:
                    d.resolve(0, pd, sid, c)
                assert e.value.code == want, (pd, sid, c)
                codes.add(want)
            else:
                assert d.resolve(0, pd, sid, c) == want, (pd, sid, c)
                kinds.add(want["kind"])
    assert codes == {M.NO_SUBCH, M.NO_COMPONENT, M.NO_SERVICE} and kinds == {"DABPLUS", "PACKET", "MP2"}
    d.push(cs.frames([[svc(0x4444, [cs.comp(3, 10)])]]))
    with pytest.raises(dab.DirUnresolved) as e:
        d.resolve(0, 0, 0x4444, 0)
    assert e.value.code == dab.DIR_NO_PKTCOMP
    d.close()


# ---- hostile content ---------------------------------------------------------------------------------------------------------------------------
def test_hostile_content():
    rng = np.random.default_rng(8)
    streams = [np.stack([cs.frame([cs.hostile_fib(rng) for _ in range(3)], nst=int(rng.integers(0, 65))) for _ in range(64)]) for _ in range(4)]
    models = _check(streams)
    assert all(m.c["facts"] > 100 and m.c["figs_truncated"] > 30 and m.c["facts_changed"] > 0 for m in models)


# ---- arrival -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["host", "device", "device+1"])
@pytest.mark.parametrize("chunk", [None, 7, "random"])
def test_arrival(how, chunk):
    _check([_rich(70, 31), _rich(41, 32), _rich(0, 33)], how=how, chunk=chunk, seed=4)


def test_reset_leaves_the_other_streams_alone():
    streams = [_rich(20, 41), _rich(20, 42), _rich(20, 43)]
    d = dab.Dir(3)
    models = _models(streams)
    _push(d, streams)
    d.reset(1)
    models[1].reset()
    for b in range(3):
        _same(d, b, models[b])
    assert cs.gpu_tuples(d, 1) == (None, [], [], [])
    more = [_rich(5, 44)] * 3
    _push(d, more)
    for b in range(3):
        models[b].push(more[b])
        _same(d, b, models[b])
    assert int(d.services(1)["first_frame"].min()) >= 20                         # the frame numbers went on
    d.close()


def test_arguments():
    d = dab.Dir(2)
    assert d.push(np.zeros(0, np.uint8), [0, 0]) == 0
    assert d.stats(1).tolist() == [0] * 11 and not d.complete(0) and d.plan(0) == []
    assert set(d.stage_ms()) == set(dab.DIR_STAGES)
    for call in (lambda: d.stats(2), lambda: d.ensemble(-1), lambda: d.reset(2), lambda: d.push(np.zeros(0, np.uint8), [-1, 0])):
        with pytest.raises(dab.DabhipError):
            call()
    d.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------
def _si_cfg(seed, **kw):
    cfg = dab.synth_preset(0, seed=seed, **kw)
    cfg.dabplus_slots, cfg.packet_slots, cfg.packet_fec_slots, cfg.ts_slots = 1 << 1, 1 << 2 | 1 << 4, 1 << 2, 1 << 3
    cfg.si_mode = 1
    return cfg


def test_end_to_end_from_iq_to_the_stages_the_plan_names():
    ntf = 40
    cfg = _si_cfg(61, cif_count0=4321)
    eng = dab.Engine(0)
    assert eng.decode([dab.synth_generate(cfg, ntf)]) > 0
    ptr, total = eng.eti_device_ptr()
    assert total >= 80
    frames = np.stack(eng.eti(0))
    d = dab.Dir(1)
    (m,) = _models([frames])
    assert d.push((ptr, [total])) == m.good == 3 * total
    _same(d, 0, m)
    assert d.complete(0) and m.c["figs_truncated"] == 0 and m.c["figs_ignored"] == 0
    plan = d.plan(0)
    # what the configuration says, slot by slot
    want = []
    for k in range(cfg.nsub):
        kind = "DABPLUS" if cfg.dabplus_slots >> k & 1 else "TS" if cfg.ts_slots >> k & 1 else "PACKET" if cfg.packet_slots >> k & 1 else "MP2"
        data = kind in ("TS", "PACKET")
        want.append({"sid": (0xE0001000 if data else 0x1000) + k, "pd": int(data), "component": 0, "label": ("SLOT %02d %s" % (k, "DAB+" if kind == "DABPLUS" else kind)).encode().ljust(16),
                     "kind": kind, "subch": cfg.sub[k].id, "fec": bool(cfg.packet_fec_slots >> k & 1),
                     "address": dab.synth_packet_addresses(cfg, k)[0] if kind == "PACKET" else 0})
    plan = sorted(plan, key=lambda p: p["sid"] & 0xFFFF)             # the directory keeps the order of first appearance; here: slot order
    assert plan == want
    e = d.ensemble(0)
    assert bytes(e["label"]) == b"DABHIP SYNTH".ljust(16) and int(e["eid"]) == cfg.eid and int(e["ecc"]) == 0xE1 and int(e["mjd"]) == 60000
    # the stages, built from the plan alone
    by_kind = {k: [p for p in plan if p["kind"] == k] for k in dab.DIR_KINDS}
    plus = dab.DabPlus(1, [p["subch"] for p in by_kind["DABPLUS"]])
    assert plus.push((ptr, [total])) > 0
    ts = dab.Ts(1, [p["subch"] for p in by_kind["TS"]])
    assert ts.push((ptr, [total])) > 0 and dict(zip(dab.TS_STATS, ts.stats(0, 0)))["rs_failed_words"] == 0
    pk = dab.Packet(1, [p["subch"] for p in by_kind["PACKET"]], fec=[p["fec"] for p in by_kind["PACKET"]])
    assert [p["fec"] for p in by_kind["PACKET"]] == [True, False] and pk.push((ptr, [total])) > 0
    for q, p in enumerate(by_kind["PACKET"]):
        recs = pk.records(0, q)
        assert len(recs) > 0 and p["address"] in set(recs["address"].tolist())
        assert dict(zip(dab.PACKET_STATS, pk.stats(0, q)))["rs_failed_codewords"] == 0
    for h in (plus, ts, pk, d):
        h.close()


def test_cli_eti2info(tmp_path):
    exe = os.path.join(os.path.dirname(dab.LIB_PATH), "eti2info")
    lab = lambda ext, sid, text, **kw: cs.fib(cs.label(ext, sid, text, **kw))
    frames = cs.frames([
        [cs.fib(cs.fig0(0, cs.e00(0x4FFF)), cs.fig0(9, cs.e09(0, 0xE2, 1))), lab(0, 0x4FFF, b"Ens\xe9mble \\ 1"), cs.fib(cs.fig0(10, cs.e10(60001, 12, 34, seconds=56, ms=789)))],
        [cs.fib(cs.fig0(1, cs.e01_short(2, 0, 35) + cs.e01_long(7, 96, 0, 2, 24) + cs.e01_short(9, 200, 0) + cs.e01_long(11, 300, 1, 0, 27))), cs.fib(cs.fig0(14, cs.e14(7, 1))),
         cs.fib(cs.fig0(3, cs.e03(5, 7, 42)))],
        [cs.fib(cs.fig0(2, cs.e02(0xD220, [cs.comp(0, 63, 2), cs.comp(0, 0, 9, ps=0)]))), lab(1, 0xD220, "Radio One", charset=6)],
        [cs.fib(cs.fig0(2, cs.e02(0xE0D22001, [cs.comp(3, 5), cs.comp(1, 24, 11, ps=0)], pd=1), pd=1)), lab(5, 0xE0D22001, "Data")],
    ])
    path = tmp_path / "in.eti"
    frames.tofile(path)

    def run(args, data):
        return subprocess.run([exe] + args, input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)

    r = run([], frames.tobytes())
    assert r.returncode == 0, r.stderr
    text = r.stdout.decode()
    assert 'ensemble EId 0x4FFF ECC 0xE2 label "Ens\\xE9mble \\x5C 1    " charset 0 time MJD 60001 12:34:56.789 UTC (frame 0)' in text
    assert "subch  2 start   0 size  96 UEP 3 128 kbit/s fec-scheme 0" in text and "subch  7 start  96 size  24 EEP 3-A  32 kbit/s fec-scheme 1" in text
    assert "subch 11 start 300 size  27 EEP 1-B  32 kbit/s fec-scheme 0" in text
    assert 'service programme 0xD220 label "Radio One       " charset 6 components 2' in text and 'service data 0xE0D22001 label "Data            " charset 0 components 2' in text
    for line in ("component 0 dabplus subch 2: eti2aac 2", "component 1 mp2 subch 9: eti2mpa 9", "component 1 ts subch 11: eti2ts 11",
                 "component 0 packet subch 7 SCId 5 address 42 DSCTy 60 DG-flag 1 fec: eti2pkt 7 --fec --address 42"):
        assert line in text, (line, text)
    assert b"eti2info: 4 frames (0 without FIC, 0 skipped), 12 FIBs (0 CRC failed), 11 FIGs (0 truncated, 0 ignored), 14 facts (0 changed, 0 dropped)" in r.stderr, r.stderr
    j = json.loads(run(["--json"], frames.tobytes()).stdout)
    assert j["complete"] is True and j["ensemble"]["eid"] == 0x4FFF and j["ensemble"]["label"] == (b"Ens\xe9mble \\ 1".ljust(16)).hex()
    assert [s["id"] for s in j["subchannels"]] == [2, 7, 9, 11] and [s["sid"] for s in j["services"]] == [0xD220, 0xE0D22001]
    assert [c["command"] for s in j["services"] for c in s["components"]] == ["eti2aac 2", "eti2mpa 9", "eti2pkt 7 --fec --address 42", "eti2ts 11"]
    # the input ends before the directory is complete: status 3; --first-complete stops at the frame that completes it
    r = run([], frames[1:].tobytes())                                             # no FIG 0/0, no ensemble label
    assert r.returncode == 3 and b"(incomplete)" in r.stdout and b"unresolved" not in r.stdout
    r = run([], frames[[0, 2, 3]].tobytes())
    assert r.returncode == 3 and r.stdout.count(b"unresolved") == 4
    r = run(["--first-complete"], np.concatenate([frames, frames[:1]]).tobytes())
    assert r.returncode == 0 and b"(incomplete)" not in r.stdout
    assert run(["--nonsense"], b"").returncode == 1
