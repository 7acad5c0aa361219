"""The EDI receiving kernels (k_edirx.hip through EdiRx) against the model of edirx_model.py, bit for bit after every call: the frames' bytes,
their records and the counters.  Packets come from the sending model (edi_model.pack of hand-built frames), so the sending kernels are not the
yardstick; only the end-to-end tests at the bottom put the engine, Edi and the command-line tools in front."""
import os
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import edi_cases as ecs
import edi_model as em
import edirx_cases as cs
import edirx_model as rx
import eti_check

pytestmark = pytest.mark.gpu

REC = ("frame", "seq", "fcth", "fct", "received", "expected", "words_filled", "erasures_filled")
IX = {k: i for i, k in enumerate(rx.STATS)}


def _gpu_out(erx, b):
    return [f.tobytes() for f in erx.frames(b)], [tuple(int(r[k]) for k in REC) for r in erx.records(b)]


def _play(nstreams, depth, script, how="host", watch=None, ctx=""):
    """script: ("push", [packets of stream 0, packets of stream 1, ..]) | ("flush", s) | ("reset", s).  Every call goes to the GPU stage and to
    one model per stream; the frames and records of the call and, at the end, the counters must be equal.  Returns the models."""
    erx = dab.EdiRx(nstreams, depth)
    models = [rx.Receiver(depth) for _ in range(nstreams)]
    watch = range(nstreams) if watch is None else watch
    for step, (op, arg) in enumerate(script):
        want = {b: [] for b in range(nstreams)}
        if op == "push":
            packets = [p for part in arg for p in part]
            counts = [len(part) for part in arg]
            if how == "host":
                n = erx.push(packets, counts)
            else:
                off = 1 if how == "device+1" else 0
                flat = np.frombuffer(b"".join(packets), np.uint8)
                buf = dab.DeviceBuffer(flat.size + 16)
                buf.upload(np.concatenate([np.zeros(off, np.uint8), flat]))
                n = erx.push((buf.ptr + off, [len(p) for p in packets], counts))
                buf.free()
            for b, part in enumerate(arg):
                want[b] = models[b].push(part)
        elif op == "flush":
            n = erx.flush(arg)
            for b in range(nstreams):
                if arg in (-1, b):
                    want[b] = models[b].flush()
        else:
            erx.reset(arg)
            models[arg].reset()
            continue
        assert n == sum(len(v) for v in want.values()), (ctx, step, op, n)
        for b in watch:
            frames, recs = _gpu_out(erx, b)
            assert recs == [x[1] for x in want[b]], (ctx, step, op, b, recs[:4], [x[1] for x in want[b]][:4])
            assert frames == [x[0].tobytes() for x in want[b]], (ctx, step, op, b)
    for b in watch:
        assert list(erx.stats(b)) == models[b].stat_list(), (ctx, b, dict(zip(rx.STATS, erx.stats(b))), dict(zip(rx.STATS, models[b].stat_list())))
    erx.close()
    return models


def _pushes(packets, how, seed=0):
    """one stream's packets as pushes: whole, one packet per push, or random cuts with empty pushes among them"""
    if how == "whole":
        return [("push", [packets])]
    if how == "each":
        return [("push", [[p]]) for p in packets]
    rng = np.random.default_rng(seed)
    out, at = [("push", [[]])], 0
    while at < len(packets):
        n = int(rng.choice([0, 1, 2, 5, 17, 60]))
        out.append(("push", [packets[at:at + n]]))
        at += n
    return out


_BORDER = {}


def _border(mode, recover, max_frag):
    key = (mode, recover, max_frag)
    if key not in _BORDER:
        frames = ecs.border_frames()
        _BORDER[key] = (cs.packets_of(frames, mode, recover, max_frag, 65534), [f.tobytes() for f in cs.expected_frames(frames)])
    return _BORDER[key]


# ---- all three modes without loss ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,recover,max_frag", cs.MODES)
def test_border_frames_without_loss_every_way_they_arrive(mode, recover, max_frag):
    """SEQ runs 65534, 65535, 0, ..: host memory in one push, device memory one packet per push, device memory off by one byte in random cuts"""
    groups, want = _border(mode, recover, max_frag)
    packets = cs.flat(groups)
    for cuts, how in (("whole", "host"), ("each", "device"), ("random", "device+1")):
        models = _play(1, 4, _pushes(packets, cuts, 7) + [("flush", -1)], how, ctx=(mode, cuts, how))
        st = models[0].stats
        assert st["frames"] == len(want) and st["packets"] == len(packets) and sum(models[0].stat_list()[1:14]) == 0
    erx = dab.EdiRx(1, 4)
    assert erx.push(packets) == len(want) and [f.tobytes() for f in erx.frames(0)] == want and erx.flush() == 0
    erx.close()


# ---- erasure counts at the edge --------------------------------------------------------------------------------------------------------------------
def test_exactly_1_47_and_48_erasures_and_one_fragment_too_many():
    rng = np.random.default_rng(48)
    script, seq, frames_out = [], 100, 0
    for l, recover, max_frag, plan, mm, drops in (
            (204, 5, 1400, (1, 204, 0, 252, 32, 8), 6, {(0, 1, 2, 3, 4, 5): 48, (0, 1, 2, 3, 4, 31): 47, (28,): 7, tuple(range(7)): None}),
            (6620, 5, 64, (32, 207, 4, 8160, 128, 64), 24, {(127,): 1, tuple(range(24)): 48, tuple(range(23)) + (127,): 47, tuple(range(25)): None})):
        assert em.plan(l, 2, recover, max_frag) == plan and rx.m_max(plan[1], plan[4]) == mm
        for dropped, most in drops.items():
            frame = ecs.frame_of_l(rng, l, seq % 250)
            group = cs.packets_of([frame], 2, recover, max_frag, seq)[0]
            counts = cs.erasure_counts(l, recover, max_frag, dropped)
            if most is None:
                assert len(dropped) == mm + 1                         # one fragment more than m_max: lost, whatever its words would need
            else:
                assert most in counts and max(counts) <= 48, (l, dropped, counts)                # some word has exactly that many
                frames_out += 1
            script.append(("push", [cs.drop(group, dropped)]))
            seq += 1
        # the next frame, whole
        script.append(("push", [cs.packets_of([ecs.frame_of_l(rng, 212, seq % 250)], 2, 1, 255, seq)[0]]))
        seq += 1
        frames_out += 1
    models = _play(1, 2, script + [("flush", 0)], "device+1", ctx="edge")
    st = models[0].stats
    assert st["frames"] == frames_out and st["groups_incomplete"] == 2 and st["groups_rs_failed"] == 0 and st["erasures_filled"] > 48 * 2


@pytest.mark.parametrize("recover", range(6))
def test_size_rule_borders_with_first_last_and_random_fragments_dropped(recover):
    rng = np.random.default_rng(recover)
    packets, seq = [], 65500
    for l in (212, 420, 828, 5796, 6412) + tuple(ecs.size_borders(recover, 255).values()):
        for pattern in ("first", "last", "random"):
            max_frag = 255 if l < 5000 else 1400
            group = cs.packets_of([ecs.frame_of_l(rng, l, seq % 250)], 2, recover, max_frag, seq & 0xFFFF)[0]
            f = len(group)
            dropped = {"first": range(recover), "last": range(f - recover, f), "random": rng.choice(f, recover, replace=False).tolist()}[pattern]
            assert max(cs.erasure_counts(l, recover, max_frag, dropped)) <= 48
            packets += cs.drop(group, dropped)
            seq += 1
    models = _play(1, 3, [("push", [packets]), ("flush", -1)], "device", ctx=recover)
    st = models[0].stats
    assert st["frames"] == seq - 65500 and (st["words_filled"] > 0) == (recover > 0) and st["groups_incomplete"] == 0


# ---- payload damage --------------------------------------------------------------------------------------------------------------------------------
def test_payload_damage_and_bad_headers():
    frames = cs.small_stream(12, 21, 240)
    g = cs.packets_of(frames, 2, 2, 64, 65530)
    assert all(len(x) >= 6 for x in g[1:])
    af = cs.packets_of(frames, 0, seq0=30)
    pf = cs.packets_of(frames, 1, 0, 64, 60)
    p = []
    p += g[0]
    p += [cs.with_byte_flipped(g[1][0], 16)] + g[1][1:]                      # nothing lost, a data byte flipped: the words are not looked at, the CRC fails
    p += cs.drop(g[2][:3] + [cs.with_byte_flipped(g[2][3], 30)] + g[2][4:], [0])   # one fragment lost, one byte flipped elsewhere: RS fails
    p += g[3][:1] + [cs.with_byte_flipped(g[3][1], 15)] + g[3][1:]          # a flipped HCRC: bad; its good copy follows
    p += [b"QF" + g[4][0][2:]] + g[4]                                        # a wrong magic
    p += [g[5][0][:-1], g[5][0] + b"\x00"] + g[5]                            # n one short and one long
    p += [cs.rehead(g[6][1], findex=len(g[6])), cs.rehead(g[6][1], fcount=257, findex=0)] + g[6]
    p += g[7][:2] + [cs.rehead(g[7][2], rsk=rx.check_packet(g[7][2])["rsk"] - 1)] + g[7][2:]    # an RSk that differs from its group's
    p += g[8][:3] + [g[8][1]] + g[8][3:]                                     # the same fragment twice
    p += g[9][:1] + [cs.with_byte_flipped(g[9][1], 16)] + g[9][2:]           # and in another fragment
    models = _play(1, 4, [("push", [p]), ("flush", -1), ("push", [cs.flat(af[:3]) + [cs.with_byte_flipped(af[3][0], 40)] + cs.flat(af[4:6])]), ("flush", -1),
                          ("push", [cs.flat(pf[:2]) + [cs.with_byte_flipped(pf[2][0], 20)] + pf[2][1:]]), ("flush", -1)], ctx="damage")
    st = models[0].stats
    assert (st["groups_crc_failed"], st["groups_rs_failed"], st["bad_packets"], st["mismatched"], st["duplicates"]) == (4, 1, 6, 1, 1), st
    assert st["frames"] == 10 - 3 + 5 + 2


# ---- order -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 4, 16])
def test_fragments_shuffled_within_depth_groups(depth):
    frames = cs.small_stream(40, depth, 230)
    want = [f.tobytes() for f in cs.expected_frames(frames)]
    groups = cs.packets_of(frames, 2, 1, 64, 65520)
    rng = np.random.default_rng(depth)
    packets = [groups[0][0]]                                                 # the first packet sets the window
    rest = [groups[0][1:]] + groups[1:]
    for a in range(0, len(rest), depth):
        part = cs.flat(rest[a:a + depth])
        packets += [part[i] for i in rng.permutation(len(part))]
    models = _play(1, depth, _pushes(packets, "random", depth) + [("flush", -1)], "device", ctx=depth)
    assert models[0].stats["frames"] == 40 and models[0].stats["late"] == 0
    erx = dab.EdiRx(1, depth)
    erx.push(packets)
    got = [f.tobytes() for f in erx.frames(0)]
    erx.flush()
    assert got + [f.tobytes() for f in erx.frames(0)] == want
    erx.close()


def test_late_fragments_a_jump_in_seq_and_swapped_af_packets():
    frames = cs.small_stream(12, 33, 245)
    g = cs.packets_of(frames, 2, 1, 64, 65534)                               # m_max 2 for these
    assert all(rx.m_max(rx.check_packet(x[0])["rsk"], len(x)) == 2 and len(x) >= 4 for x in g[1:6])
    held1, held3 = g[1][0], g[3][:3]
    p = g[0] + g[1][1:] + g[2] + g[3][3:] + cs.flat(g[4:8]) + [held1] + held3 + cs.flat(g[8:])
    models = _play(1, 2, [("push", [p]), ("flush", 0)], ctx="late")
    st = models[0].stats
    assert st["late"] == 4 and st["groups_incomplete"] == 1 and st["frames"] == 11 and st["words_filled"] >= 1
    af = cs.flat(cs.packets_of(frames, 0, seq0=65534))
    swapped = [af[0]] + [af[1 + (i ^ 1)] for i in range(10)] + [af[11]]
    far = cs.flat(cs.packets_of(frames[:3], 1, 0, 64, 20010))
    models = _play(2, 4, [("push", [swapped, af[:4] + far]), ("flush", -1)], "device", ctx="swap")
    assert models[0].stats["frames"] == 12 and models[0].stats["late"] == 0
    assert models[1].stats["frames"] == 7 and models[1].stats["missing"] > 20000


# ---- state -----------------------------------------------------------------------------------------------------------------------------------------
def test_state_over_pushes_flush_reset_and_streams_of_unequal_length():
    rng = np.random.default_rng(5)
    lens = (65, 0, 1, 33, 7)
    streams = []
    for b, n in enumerate(lens):
        groups = cs.packets_of(cs.small_stream(n, 50 + b, 200 + 9 * b), b % 3, 1, 64, 65500 + b) if n else []
        streams.append(cs.flat([cs.drop(x, [int(rng.integers(0, len(x)))]) if b % 3 == 2 and len(x) > 3 and i % 2 else x for i, x in enumerate(groups)]))
    script, at = [], [0] * 5
    sizes = [3, 0, 1, 40, 2, 1000]
    for k, n in enumerate(sizes):                                            # groups cut anywhere: their fragments arrive over several pushes
        script.append(("push", [s[a:a + n] for s, a in zip(streams, at)]))
        at = [a + n for a in at]
        if k == 2:
            script.append(("flush", 3))                                     # flush, then more packets: what was flushed comes late
        if k == 3:
            script.append(("reset", 0))                                     # the window of stream 0 forgets; its numbers go on
    script += [("flush", -1), ("push", [[], [], [], [], []]), ("flush", 4)]
    models = _play(5, 3, script, "device+1", ctx="state")
    assert models[0].stats["frames"] > 30 and models[1].stat_list() == [0] * 15 and models[2].stats["frames"] == 1
    # a group whose fragments arrive over three pushes
    g = cs.packets_of(cs.small_stream(2, 77), 2, 2, 64, 5)
    _play(1, 4, [("push", [g[1][:2]]), ("push", [g[1][2:4] + g[0]]), ("push", [g[1][4:]]), ("flush", 0)], ctx="three")


@pytest.mark.parametrize("nstreams", [257, 1025])
def test_many_streams_of_three_frames(nstreams):
    short = []
    for b in range(7):
        groups = cs.packets_of(cs.small_stream(3, 90 + b, 248), b % 3, 1, 255, 65534)
        short.append(cs.flat(groups[:-1]) + cs.drop(groups[-1], [0] if b % 3 == 2 else []))
    watch = sorted(set(list(range(0, nstreams, 13)) + [nstreams - 2, nstreams - 1]))
    _play(nstreams, 2, [("push", [short[b % 7] for b in range(nstreams)]), ("flush", -1)], "host", watch=watch, ctx=nstreams)


def test_stage_times_empty_pushes_and_refusals():
    erx = dab.EdiRx(2, 4)
    assert erx.push([], [0, 0]) == 0 and erx.flush() == 0
    assert tuple(erx.stage_ms()) == dab.EDIRX_STAGES and all(v >= 0 for v in erx.stage_ms().values())
    assert erx.records(1).size == 0 and erx.frames(0).shape == (0, 6144) and list(erx.stats(1)) == [0] * 15
    af = cs.flat(cs.packets_of(cs.small_stream(3, 1), 0))
    assert erx.push(af, [3, 0]) == 3 and erx.push([], [0, 0]) == 0 and erx.frames(0).shape[0] == 0
    for call in (lambda: erx.records(2), lambda: erx.frames(-1), lambda: erx.stats(2), lambda: erx.flush(2), lambda: erx.reset(-1), lambda: erx.push([], [-1, 0]),
                 lambda: erx.push((0, [5], [1, 0])), lambda: erx.push((1, [-5], [1, 0]))):
        with pytest.raises(dab.DabhipError):
            call()
    erx.close()
    for args in ((0,), (1, 0), (1, 17), (1 << 17, 4)):
        with pytest.raises(dab.DabhipError):
            dab.EdiRx(*args)


# ---- foreign items ---------------------------------------------------------------------------------------------------------------------------------
def test_foreign_items_time_stamp_and_rfud():
    rng = np.random.default_rng(11)
    frames = [ecs.frame(rng, 9 + i, [4, 2, 0, 7][:1 + i % 4], ficf=i % 3 != 2, mid=1) for i in range(8)]
    afs = [cs.make_af(frames[0], 0, between=[(b"*dmy", bytes(5)), (b"avtm", b"xyz")]), cs.make_af(frames[1], 1, atst=bytes(range(8))),
           cs.make_af(frames[2], 2, rfud=b"\x01\x02\x03"), cs.make_af(frames[3], 3, atst=bytes(8), rfud=bytes(3), between=[(b"*dmy", b"")]), cs.make_af(frames[4], 4, ptr=False),
           cs.make_af(frames[5], 5, between=[(b"est\x07", bytes(3))]), cs.make_af(frames[6], 6, atst=bytes(7)), cs.make_af(frames[7], 7, between=[(b"*ptr", b"DETJ" + bytes(4))])]
    packets = []
    for i, a in enumerate(afs):
        packets += cs.fragment(a, i, i % 3, 1, 64)
    models = _play(1, 4, [("push", [packets]), ("flush", -1)], "device+1", ctx="foreign")
    st = models[0].stats
    assert (st["frames"], st["groups_refused"], st["items_ignored"], st["with_atst"]) == (5, 3, 3, 2)
    erx = dab.EdiRx(1, 4)
    erx.push(packets)
    assert [f.tobytes() for f in erx.frames(0)] == [rx.rebuild(em.carried(f)).tobytes() for f in frames[:5]]
    erx.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_engine_edi_two_fragments_lost_edirx():
    cfgs = [dab.synth_preset(0, seed=910 + b, cif_count0=(4990 + 1200 * b) % 5000, skip_samples=7000 * b) for b in range(2)]
    eng = dab.Engine(0)
    assert eng.decode([dab.synth_generate(c, 24) for c in cfgs]) > 0
    ptr, total = eng.eti_device_ptr()
    counts = [eng.eti_count(b) for b in range(2)]
    edi = dab.Edi(2, dab.EDI_PFT_FEC, 2, 1400)
    assert edi.push((ptr, counts)) > 0
    packets, per_stream = [], []
    for b in range(2):
        data, recs = edi.data(b).tobytes(), edi.records(b)
        f = int(recs[0]["fcount"])
        kept = [data[int(r["offset"]):int(r["offset"]) + int(r["length"])] for r in recs if int(r["findex"]) not in (1, f - 1)]
        per_stream.append(len(kept))
        packets += kept
    edi.close()
    erx = dab.EdiRx(2, 4)
    assert erx.push(packets, per_stream) + erx.flush() == sum(counts)
    erx.close()
    erx = dab.EdiRx(2, 1)                                                    # depth 1: every frame comes with the first packet of the next, the last with the flush
    n = erx.push(packets, per_stream)
    got = [erx.frames(b) for b in range(2)]
    recs = [erx.records(b) for b in range(2)]
    assert n == sum(counts) - 2 and erx.flush() == 2
    for b in range(2):
        want = eng.eti(b)
        frames = np.concatenate([got[b], erx.frames(b)])
        assert frames.shape == want.shape and (frames == want).all()
        assert all(eti_check.parse(f)["nst"] == cfgs[b].nsub for f in frames)
        assert (recs[b]["received"] == recs[b]["expected"] - 2).all() and (recs[b]["words_filled"] > 0).all()
    assert erx.stats(0)[IX["erasures_filled"]] > 0 and erx.stats(0)[IX["groups_rs_failed"]] == 0
    erx.close()


def test_cli_dab2eti_pipe_eti2edi_pipe_edi2eti(tmp_path):
    here = os.path.dirname(dab.LIB_PATH)
    exe = lambda name: os.path.join(here, name)
    cfg = dab.synth_preset(0, seed=78, cif_count0=4995)
    cap = tmp_path / "cap.cu8"
    dab.synth_generate(cfg, 24).tofile(cap)
    eti = subprocess.run([exe("dab2eti-hip"), str(cap)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True, timeout=300).stdout
    nframes = len(eti) // 6144
    assert nframes >= 20
    run = subprocess.run(["bash", "-c", "set -o pipefail; '%s' '%s' | '%s' --fec 2 | '%s'" % (exe("dab2eti-hip"), cap, exe("eti2edi"), exe("edi2eti"))],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert run.returncode == 0 and run.stdout == eti, run.stderr
    assert b"edi2eti: %d frames, 0 bytes skipped" % nframes in run.stderr, run.stderr
    # the same packets in a file, garbage spliced between them (some of it beginning like a packet)
    frames = list(np.frombuffer(eti, np.uint8).reshape(-1, 6144))
    packets = cs.flat(cs.packets_of(frames, 2, 2, 1400))
    junk = [b"", b"\x00", b"PF" + bytes(20), b"AF" + bytes(5), b"xyzPFAF" * 3]
    spliced = b"".join(junk[i % 5] + p for i, p in enumerate(packets)) + b"tail"
    skipped = sum(len(junk[i % 5]) for i in range(len(packets))) + 4
    path = tmp_path / "in.edi"
    path.write_bytes(spliced)
    run = subprocess.run([exe("edi2eti"), "--depth", "2", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert run.returncode == 0 and run.stdout == eti, run.stderr
    assert b"edi2eti: %d frames, %d bytes skipped" % (nframes, skipped) in run.stderr, run.stderr
    for bad in (["--depth", "0"], ["--depth", "17"], ["--depth"], ["--nonsense"], ["a", "b"]):
        run = subprocess.run([exe("edi2eti")] + bad, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert run.returncode == 1 and run.stderr.startswith(b"Usage: edi2eti"), bad
