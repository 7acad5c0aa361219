"""Transmitter identification on the GPU (include/dabhip.h, "TII"; csrc/k_tii.hip, csrc/tii.cpp): the stage entry against the numpy model
(tests/tii_model.py) bit for bit -- 1, 3 and 65 frames, every window start and step of the list, all-0 and all-255 frames, host and device
pointers --; the engine's sums against the model fed the frame buffers rebuilt from the trace, the identifiers found, ETI bytes and traces with TII
on and off; a session in odd segments against the one-shot decode; and the CLI's --tii."""
import functools
import os
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import tii_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dabtools_amd", "dab2eti-hip")
TFB = dab.TF_BYTES
W0S = (0, 304, 608)
STEPS = (0, 1, 0x6b8b4567, 1 << 31, (1 << 32) - 1)
NTF = 10


@pytest.fixture(scope="module")
def engine():
    e = dab.Engine(0)
    yield e
    e.close()


def stage_case(nframes):
    """Frames, window starts and steps: every (w0, step) pair occurs from 15 frames on; of 65 frames the first 15 are all 0 bytes and the next 15 all
    255 (full scale on both rails through every pair), of 3 frames the first two."""
    rng = np.random.default_rng(nframes)
    frames = rng.integers(0, 256, (nframes, TFB), dtype=np.uint8)
    j = np.arange(nframes)
    if nframes >= 3:
        edge = 15 if nframes >= 30 else 1
        frames[:edge], frames[edge:2 * edge] = 0, 255
    w0 = np.array(W0S)[(j + nframes) % 3]
    step = np.array(STEPS, dtype=np.uint64)[(j // 3 + nframes) % 5]
    return frames, w0, step


@pytest.mark.gpu
@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("nframes", [1, 3, 65])
def test_stage_bit_exact_against_the_model(engine, nframes, on_device):
    frames, w0, step = stage_case(nframes)
    want = tm.frame_sums(frames, w0, step)
    if on_device:
        buf = dab.DeviceBuffer(frames.size)
        buf.upload(frames)
        got = engine.stage_tii(None, w0, step, device_ptr=buf.ptr)
        buf.free()
    else:
        got = engine.stage_tii(frames, w0, step)
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:4]
    if nframes == 65:
        assert {(int(a), int(s)) for a, s in zip(w0[:15], step[:15])} == {(a, s) for a in W0S for s in STEPS}
        assert got[:30].any() and got[30:].all()


@pytest.mark.gpu
def test_stage_refusals(engine):
    frame = np.zeros(TFB, np.uint8)
    for w0 in (-1, 609):
        with pytest.raises(dab.DabhipError, match="w0 must be 0 .. 608"):
            engine.stage_tii(frame, [w0], [0])


# ---- the engine ---------------------------------------------------------------------------------------------------------------------------------
# "two": 10 dB apart at 9 dB of SNR, the weaker one at the level of a data carrier -- the rule compares a comb with the bins around it and does not
# subtract the noise floor, so a comb 10 dB below a data carrier is out of reach at 9 dB however many frames are folded (the header's "Reach")
COMBS = {"one": ((17, 5, 0.0),), "two": ((3, 1, 10.0), (40, 9, 0.0)), "cfo": ((61, 22, 0.0),), "none": ()}


@functools.lru_cache(maxsize=None)
def capture(name, cfo=0.0, ntf=NTF):
    snr, skip = (9.0, 100000) if name == "two" else (1000.0, 0)
    cfg = dab.synth_preset(1, seed=5 + len(name), snr_db=snr, skip_samples=skip, cfo_hz=cfo)
    cfg.set_tii(COMBS[name])
    iq = dab.synth_generate(cfg, ntf)
    iq.setflags(write=False)
    return iq


def model_sums(e, b, iq):
    """The model fed what the engine's front end saw: the frame buffer of every call rebuilt from the trace's shifts (dabhip_host_fifo_call), its
    window cut at 304 + fine_timeshift, its step from the trace's frequency estimates."""
    ncalls = iq.size // dab.CHUNK_BYTES
    ints, ffs = e.trace(b, ncalls)
    nco = e.trace_nco(b, ncalls)
    fifo = dab.HostFifo()
    coarse = fine = 0
    windows, steps = [], []
    for k in range(len(ints)):
        status, view, _ = fifo.call(coarse, fine, iq)
        assert (status > 0) == bool(ints[k][1])                   # the FIFO's own status: a frame was read
        if tm.counted(ints[k][0], ints[k][3], ffs[k]):
            buf = dab.HostFifo.materialise(iq, view, fifo.tail).reshape(-1, 2)
            w0 = tm.W0 + int(ints[k][3])
            windows.append(buf[w0:w0 + tm.S])
            steps.append(tm.step_of(ints[k][4], ffs[k], nco[k]))
        coarse, fine = int(ints[k][2]), int(ints[k][3])
    fifo.close()
    T = tm.window_sums(np.array(windows).reshape(-1, tm.S, 2), steps).sum(axis=0, dtype=np.uint64) if windows else np.zeros(192, np.uint64)
    return T, len(windows)


def decode(e, iqs, tii):
    e.set_tii(tii)
    n = e.decode(iqs)
    out = []
    for b, iq in enumerate(iqs):
        ncalls = iq.size // dab.CHUNK_BYTES
        out.append((e.eti(b).tobytes(), e.trace(b, ncalls)[0].tobytes(), e.trace(b, ncalls)[1].tobytes()))
    return n, out


def check_ids(found, want):
    """The configured identifiers unflagged, anything else only with SHADOW."""
    assert sorted((r["main"], r["sub"]) for r in found if not r["shadow"]) == sorted((m, s) for m, s, _ in want), found


@pytest.mark.gpu
def test_engine_sums_identifiers_and_unchanged_output(engine):
    names = ("one", "two", "cfo", "none")
    iqs = [capture("one"), capture("two"), capture("cfo", 300.0), capture("none")]
    n_off, off = decode(engine, iqs, False)
    with pytest.raises(dab.DabhipError):
        engine.tii_sums(0)                                        # never switched on: no sums
    n_on, on = decode(engine, iqs, True)
    assert n_on == n_off and on == off                            # ETI bytes and traces are those of a decode without it
    assert "tii" not in engine.stage_ms() and engine.tii_ms() > 0
    for b, name in enumerate(names):
        T, frames = engine.tii_sums(b)
        want, counted = model_sums(engine, b, iqs[b])
        print(name, "frames", frames, engine.tii(b))
        assert frames == counted and frames >= 5                  # of 10 TF: one read is dropped, the skipped capture loses two more to its time search
        assert np.array_equal(T, want), (name, np.flatnonzero(T != want)[:8])
        assert engine.tii(b) == dab.tii_detect(T) == tm.detect(T)
        check_ids(engine.tii(b), COMBS[name])
    assert engine.tii(3) == []
    engine.set_tii(False)
    n_again, again = decode(engine, iqs, False)
    assert n_again == n_off and again == off and engine.tii_ms() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("cfo, afc", [(-1200.0, False), (300.0, True)])
def test_engine_under_a_carrier_offset(cfo, afc):
    """-1200 Hz: the coarse estimate is -1 carrier and the fine one carries the rest; +300 Hz with the software AFC: the NCO's frequency enters the
    step."""
    e = dab.Engine(0)
    e.set_afc(afc)
    e.set_tii(True)
    iq = capture("cfo", cfo)
    e.decode([iq])
    ncalls = iq.size // dab.CHUNK_BYTES
    ints, ffs = e.trace(0, ncalls)
    ok = ints[:, 0] == 1
    if afc:
        assert e.trace_nco(0, ncalls)[ok].any()
    else:
        assert (ints[ok, 4] == -1).any()
    T, frames = e.tii_sums(0)
    want, counted = model_sums(e, 0, iq)
    assert frames == counted > 0 and np.array_equal(T, want)
    print(cfo, afc, e.tii(0))
    check_ids(e.tii(0), COMBS["cfo"])
    e.close()


@pytest.mark.gpu
def test_session_in_odd_segments(engine):
    iqs = [capture("one"), capture("two")]
    engine.set_tii(True)
    engine.decode(iqs)
    want = [engine.tii_sums(b) for b in range(2)]
    engine.set_tii(False)
    s = dab.Stream(2)
    s.set_tii(True)
    cuts = [0, 262144 + 7 * 2, 3 * 262144 - 2, 1000001 * 2, 2500000, iqs[1].size, iqs[0].size]
    for a, b in zip(cuts, cuts[1:]):
        s.feed([iq[min(a, iq.size):min(b, iq.size)] for iq in iqs])
    for b in range(2):
        T, frames = s.tii_sums(b)
        assert frames == want[b][1] and np.array_equal(T, want[b][0]), b
        assert s.tii(b) == dab.tii_detect(T)
    s.tii_reset()
    for b in range(2):
        T, frames = s.tii_sums(b)
        assert frames == 0 and not T.any() and s.tii(b) == []
    s.close()


@pytest.mark.gpu
def test_device_modulator_refuses_tii():
    cfg = dab.synth_preset(1, seed=1)
    cfg.set_tii([(1, 2, 0.0)])
    buf = dab.DeviceBuffer(dab.synth_bytes(cfg, 1))
    with pytest.raises(dab.DabhipError, match="TII combs .* host generator only"):
        dab.synth_generate_device([cfg], 1, [buf.ptr])
    cfg.set_tii([])
    dab.synth_generate_device([cfg], 1, [buf.ptr])
    buf.free()


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli(tmp_path):
    paths = []
    for name in ("one", "none"):                                  # 16 TF: long enough to lock, so that stdout carries frames
        paths.append(str(tmp_path / (name + ".cu8")))
        capture(name, 0.0, 16).tofile(paths[-1])
    plain = subprocess.run([CLI] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    tii = subprocess.run([CLI, "--tii"] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert plain.returncode == 0 and tii.returncode == 0, tii.stderr[-2000:]
    assert tii.stdout == plain.stdout and len(plain.stdout) > 0
    lines = [l for l in tii.stderr.decode().splitlines() if "TII:" in l]
    assert lines == ["%s: TII: main=17 sub=05 level=0.0dB" % paths[0]], tii.stderr.decode()
    assert b"TII:" not in plain.stderr
    session = subprocess.run([CLI, "--tii", "--stream", "--segment-calls", "5", paths[0]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert session.returncode == 0 and session.stdout == plain.stdout[:len(session.stdout)] and len(session.stdout) > 0
    assert [l for l in session.stderr.decode().splitlines() if "TII:" in l] == ["TII: main=17 sub=05 level=0.0dB"], session.stderr.decode()
    two = subprocess.run([CLI, "--tii", "--devices", "0,0"] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert two.returncode == 1 and two.stdout == b"" and b"--tii runs on one device" in two.stderr
