"""The MPEG-2 TS model (tests/ts_model.py) on the CPU: its RS(204,188) against long division and against the independent decoder of
rs204_reference.py on every crafted word, the closed-form de-interleaver against a FIFO (Forney) interleaver written out here, the sync rule
on crafted streams whose results the construction fixes, independence of how a stream is cut into pushes, the modulator's TS content, and
tests/host_sanitize/ts_units.cpp, a stand-alone program, under ASan + UBSan: ts_chunk_step against the rule slot by slot, the position map, and
the bound on a push's units per lane as a property over every STL, carried count and push size."""
import os
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import packet_cases as pcs
import rs204_reference as ref
import ts_cases as cs
import ts_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- Reed-Solomon ----------------------------------------------------------------------------------------------------------------------------------
def test_parity_against_long_division():
    rng = np.random.default_rng(1)
    src = cs.Source(rng)
    for _ in range(20):
        w = src.word()
        assert w[0] == m.SYNC and (w[m.K:] == ref.encode(w[:m.K])).all()
        assert not any(ref.syndromes(w))


def test_decoder_against_the_independent_one_on_every_crafted_word():
    """Every crafted error pattern on a transport packet's code word: the model's decoder and rs204_reference.decode agree on the word and the
    count, and where the construction fixes the result it is that."""
    rng = np.random.default_rng(2)
    src = cs.Source(rng)
    cases = pcs.rs_cases()
    seen = 0
    for cls in sorted(cases):
        for label, rx0, want0, n, err in cases[cls]:
            w = src.word()
            rx = w ^ err
            got, count = m.rs_decode(rx)
            rgot, rcount = ref.decode(rx)
            assert count == rcount and (got == rgot).all(), (cls, label, count, rcount)
            if n is not None:                                  # the code is linear: the pattern's fate does not depend on the code word
                assert count == n, (cls, label)
                assert (got == (rx if n < 0 else rx ^ (rx0 ^ want0))).all(), (cls, label)
            seen += 1
    assert seen > 350
    for cls, lo in (("e1", 5), ("e8", 12), ("e9", 12), ("parity", 3), ("miscorrect", 8), ("shortened", 10), ("beyond", 300), ("clean", 3)):
        assert len(cases[cls]) >= lo
    assert any(err[0] for c in cases["e1"] + cases["e8"] for err in [c[4]])           # an error in byte 0 among them


# ---- the interleaver -------------------------------------------------------------------------------------------------------------------------------
def fifo_interleave(stream_in):
    """The convolutional byte interleaver with twelve delay lines of 17 j bytes (j = 0..11), byte by byte: input byte i goes through branch
    i mod 12; the lines start full of zeros."""
    lines = [[0] * (17 * j) for j in range(12)]
    out = np.zeros(len(stream_in), dtype=np.uint8)
    for i, b in enumerate(stream_in):
        line = lines[i % 12]
        if line:
            line.append(int(b))
            out[i] = line.pop(0)
        else:
            out[i] = b
    return out


def test_closed_form_gather_against_a_fifo_interleaver():
    rng = np.random.default_rng(3)
    words = cs.Source(rng).words(49 + 11)
    sent = fifo_interleave(words.reshape(-1))                # word n's slot starts at 204 n: phase 0
    mismatches = 0
    for n in range(49):                                      # the words whose 2448 bytes are all there
        mismatches += int((sent[m.SLOT * n + m.GATHER] != words[n]).sum())
    assert mismatches == 0
    # and the model's own interleaver is that FIFO, wherever the lines have filled (17 * 11 * 12 = 2244 bytes in)
    mine = m.interleave(np.concatenate([np.zeros((11, m.N), np.uint8), words]), -11, 0, sent.size)
    assert (mine[2244:] == sent[2244:]).all()
    assert all(m.GATHER[k] == k + 204 * (k % 12) for k in range(m.N)) and m.GATHER[0] == 0


# ---- the sync rule ---------------------------------------------------------------------------------------------------------------------------------
def _cuts(nframes, how, rng):
    if how == "one":
        return [nframes]
    if how == "each":
        return [1] * nframes
    out, left = [0, 1], nframes - 1
    while left > 0:
        out.append(min(int(rng.choice([0, 1, 2, 3, 5, 7, 12, 30])), left))
        left -= out[-1]
    return out


def _lane(frames, scid, how, seed=0):
    rng = np.random.default_rng(seed)
    lane, recs, data, at = m.Lane(scid), [], [], 0
    for n in _cuts(len(frames), how, rng):
        r, d = lane.push(frames[at:at + n])
        at += n
        recs += r
        data.append(d)
    return recs, np.concatenate(data), lane


def _same_under_every_cutting(frames, scid=cs.SYNC_ID):
    recs, data, lane = _lane(frames, scid, "one")
    for how in ("each", "random"):
        r2, d2, l2 = _lane(frames, scid, how, seed=len(frames))
        assert r2 == recs and (d2 == data).all() and l2.stat_list() == lane.stat_list(), how
        assert l2.max_carry <= m.CARRY
    return recs, data, lane


@pytest.mark.parametrize("name", sorted(cs.sync_streams()))
def test_sync_rule_on_crafted_streams(name):
    stream, want = cs.sync_streams()[name]
    recs, data, lane = _same_under_every_cutting(cs.sync_frames(stream))
    for k, v in want.items():
        assert lane.stats[k] == v, (name, k, lane.stats)
    assert lane.stats["packets"] == len(recs) > 30
    # only a slip can break words: the 12 whose 2448 bytes span the cut, and the 2 taken as misses on the old grid behind it
    assert lane.stats["rs_failed_words"] <= (14 if name.startswith("slip") else 0), lane.stats


def test_run_decided_with_its_last_byte_and_carried_one_byte_later():
    """After three frames of 408 bytes the run whose 5th byte is byte 1223 is decided (the lane is synced and carries from the run's start); the
    one whose 5th byte is byte 1224 is not (the lane carries the last 816 bytes)."""
    streams = cs.sync_streams()
    for name, synced, carried in (("run ends with the push", True, m.RUN_SPAN + 1), ("run ends one byte later", False, m.RUN_SPAN)):
        lane = m.Lane(cs.SYNC_ID)
        recs, _ = lane.push(cs.sync_frames(streams[name][0])[:3])
        assert not recs and lane.synced == synced and len(lane.buf) == carried, (name, lane.synced, len(lane.buf))


def test_every_kind_of_break():
    frames, losses = cs.broken_frames()
    recs, data, lane = _same_under_every_cutting(frames)
    assert lane.stats["sync_losses"] == losses, lane.stats
    assert lane.stats["rs_failed_words"] == 0 and lane.stats["bad_sync_packets"] == 0 and lane.stats["packets"] > 100, lane.stats
    pos = [r[0] for r in recs]
    assert pos == sorted(pos) and lane.base + len(lane.buf) == sum(8 * (cs.SYNC_STL if i not in range(95, 125) else 26) for i in range(150) if i not in (20, 45, 70, 126))


def test_rs_words_in_a_stream():
    stream, npat = cs.rs_stream(np.random.default_rng(5))
    frames = cs.frames_of_bytes(3, [(6, 204, stream)])
    recs, data, lane = _same_under_every_cutting(frames, scid=6)
    st = lane.stats
    assert st["sync_losses"] == 0 and st["packets"] >= 2 * npat
    assert st["rs_failed_words"] >= 10 + 290 and st["rs_corrected_bytes"] >= 12 * 8 + 5 + 13 + 8 * 8, st
    assert st["from_missed_slots"] > 0 and st["bad_sync_packets"] > 0, st


# ---- the modulator -----------------------------------------------------------------------------------------------------------------------------------
def _ts_cfg(seed, phase=0, mask=None):
    cfg = dab.synth_preset(1, seed=seed)
    cfg.ts_slots = (1 << cfg.nsub) - 1 if mask is None else mask
    cfg.ts_phase = phase
    return cfg


def test_modulator_is_off_by_default_and_leaves_the_other_slots_alone():
    plain = dab.synth_preset(1, seed=9)
    assert plain.ts_slots == 0 and plain.ts_phase == 0 and plain.ts_pad == 0
    cfg = _ts_cfg(9, 0, 1 << 2)
    for cif in (0, 7, 300):
        assert (dab.synth_fibs(cfg, cif) == dab.synth_fibs(plain, cif)).all()
        for slot in range(plain.nsub):
            same = (dab.synth_payload(cfg, cif, slot) == dab.synth_payload(plain, cif, slot)).all()
            assert same == (slot != 2), (cif, slot)
    assert (dab.synth_generate(dab.synth_preset(1, seed=9), 2) == dab.synth_generate(plain, 2)).all()


def test_modulator_bytes_against_the_models_interleaver():
    for phase in (0, 77, 203, 2500):
        cfg = _ts_cfg(31 + phase, phase)
        for slot in range(cfg.nsub):
            ncif = max(12, -(-16000 // dab.synth_payload(cfg, 0, slot).size))
            stream = np.concatenate([dab.synth_payload(cfg, cif, slot) for cif in range(ncif)])
            first, count = m.words_needed(phase, stream.size)
            words = np.stack([dab.synth_ts_word(cfg, slot, first + i) for i in range(count)])
            assert first < 0 and (m.interleave(words, first, phase, stream.size) == stream).all(), (phase, slot)
            assert not m.syndromes_many(words).any() and (words[:, 0] == m.SYNC).all()
            # two or three PIDs and null packets, a continuity counter per PID that counts on across blocks and through n = 0
            pids = (words[:, 1].astype(int) & 0x1F) << 8 | words[:, 2]
            kinds = sorted(set(pids.tolist()))
            assert kinds[-1] == m.NULL_PID and len(kinds) in (3, 4), kinds
            for pid in kinds[:-1]:
                cc = words[pids == pid, 3] & 15
                assert len(cc) > 16 and ((cc[1:] - cc[:-1]) % 16 == 1).all(), (phase, slot, pid)
            assert 0 < int(((words[:, 1] & 0x40) != 0).sum()) < count // 3
            # through the model's lane the words come back as sent
            frames = cs.frames_of_bytes(0, [(5, stream.size // ncif // 8, stream)])
            recs, data = m.Lane(5).push(frames)
            n0 = (recs[0][0] - phase) // m.SLOT
            assert len(recs) > 3 and all(r[0] == phase + m.SLOT * (n0 + i) and r[3] & ~m.PUSI == 0 for i, r in enumerate(recs))
            assert (data == words[n0 - first:n0 - first + len(recs), :m.K]).all()


def test_modulator_refusals():
    def refused(change, call=lambda c: dab.synth_payload(c, 0, 0)):
        cfg = _ts_cfg(5)
        change(cfg)
        with pytest.raises(dab.DabhipError):
            call(cfg)

    def past_nsub(c):
        c.ts_slots |= 1 << c.nsub

    def also_dabplus(c):
        c.dabplus_slots = 1

    def also_packet(c):
        c.packet_slots = 2

    refused(past_nsub)
    refused(also_dabplus)
    refused(also_packet)
    refused(lambda c: c.set_reconf(0, 40, c.multiplex()))
    refused(lambda c: None, lambda c: dab.synth_ts_word(dab.synth_preset(1, seed=5), 0, 0))     # not a TS slot
    refused(past_nsub, lambda c: dab.synth_ts_word(c, 0, 0))
    assert dab.synth_ts_word(_ts_cfg(5), 0, -3).size == 204


def test_ts_create_needs_a_gpu_or_says_so():
    try:
        t = dab.Ts(1, [3])
    except dab.DabhipError as e:
        assert "GPU" in str(e) or "HIP" in str(e)
    else:
        t.close()
    with pytest.raises(dab.DabhipError):
        dab.Ts(1, [64])


# ---- the shared header under sanitizers ------------------------------------------------------------------------------------------------------------
def test_sync_header_under_sanitizers():
    here = os.path.join(ROOT, "tests", "host_sanitize")
    os.makedirs(os.path.join(here, "build"), exist_ok=True)
    exe = os.path.join(here, "build", "ts_units_asan")
    build = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            os.path.join(here, "ts_units.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "Sanitizer" not in run.stderr, run.stderr[-4000:]
    out = run.stdout.split("\n")
    assert out[0].split() == ["ok", "ts-units"]
    # the fullest slot array of the property is full: a lane of nothing but hits gives exactly the bound; and no carry passed 2447 bytes
    words = out[1].replace(";", "").split()
    assert words[3] == "fullest" and words[4] == words[6] == "1923", out[1]     # 64 frames at STL 766 on 2447 carried bytes
    assert words[-4] == "carry" and int(words[-3]) <= m.CARRY and int(words[-3]) >= m.CARRY - 8, out[1]
