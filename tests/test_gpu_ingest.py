"""The ingest stage on the GPU (include/dabhip.h, "ingest stage"; csrc/k_ingest.hip, csrc/ingest.cpp): its bytes against the numpy model
(tests/ingest_model.py) for every format and ratio class, across pushes, at positions beyond 2^32, through the decoder and through the CLI."""
import os
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import ingest_cases as cases
import ingest_model as im
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dabtools_amd", "dab2eti-hip")
FORMATS = ("cu8", "cs8", "cs16", "cf32")
RATES = (2048000, 2400000, 2500000, 2560000, 4096000, 10000000)      # 1/1, 64/75, 512/625, 4/5, 1/2, 128/625
TILE, GROUP = 1024, 8 * 1024                                         # outputs of one workgroup's tile, and of the tiles one workgroup walks (k_ingest.hip)
W = im.W


def run_rounds(ing, models, raws, rounds):
    """rounds: per round the samples each stream pushes.  Every round's bytes and gains against the models'."""
    at = [0] * len(models)
    for sizes in rounds:
        parts = [raws[b][2 * at[b]:2 * (at[b] + n)] for b, n in enumerate(sizes)]
        total = ing.push(parts)
        want = [m.push(p) for m, p in zip(models, parts)]
        assert total == sum(w.size for w in want)
        for b, w in enumerate(want):
            got = ing.read(b)
            assert got.size == w.size, (b, sizes, got.size, w.size)
            assert np.array_equal(got, w), (b, sizes, int(np.flatnonzero(got != w)[0]))
            assert ing.gain(b) == models[b].g
        at = [a + n for a, n in zip(at, sizes)]


@pytest.mark.gpu
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_bit_exact_against_the_model(fmt, rate):
    rng = np.random.default_rng(rate // 1000 + 7 * len(fmt))
    _, L, M, T = dab.ingest_taps(fmt, rate)
    need = lambda k: cases.samples_for_outputs(L, M, T, k)
    # explicit gain: three streams of different lengths in one object.  Stream 0 walks the first output's edge (totals 0, 1, T/2 - 1, T/2, T/2 + 1),
    # stream 1 starts with T/2 + 1 samples, stream 2 with a few thousand; then pushes that complete exactly TILE - 1 / TILE / TILE + 1 and
    # GROUP - 1 / GROUP / GROUP + 1 outputs (each more than L of them: every phase), empty pushes in between.
    h = T // 2
    rounds = [[0, h + 1, 3001], [1, 0, 0], [max(h - 2, 0), 1, 1], [1, max(h - 1, 0), 0], [1, h, 2999]]
    done = [sum(r[b] for r in rounds) for b in range(3)]
    for targets in ((TILE - 1, TILE, TILE + 1), (GROUP + 1, GROUP - 1, GROUP), (0, 1, L)):
        sizes = []
        for b, k in enumerate(targets):
            have = 0 if done[b] <= h else ((done[b] - h) * L - 1) // M + 1 if T else done[b]
            n = need(have + k) - done[b] if k else 0
            sizes.append(max(n, 0))
            done[b] += sizes[-1]
        rounds.append(sizes)
    raws = [cases.random_raw(rng, fmt, done[b]) for b in range(3)]
    for gain in (256, 70000):
        ing = dab.Ingest(0, 3, fmt, rate, gain)
        run_rounds(ing, [im.IngestModel(fmt, rate, gain) for _ in range(3)], raws, rounds)
        ing.close()
    # automatic gain: the window's end inside a push (stream 0), exactly at a push's end (stream 1), in the first push (stream 2); stream 1 is quiet
    rounds = [[W - 100, W - 100, W + 3000], [3000, 100, 0], [0, 2900, 7]]
    raws = [cases.random_raw(rng, fmt, sum(r[b] for r in rounds)) for b in range(3)]
    raws[1] = (raws[1] // 16).astype(raws[1].dtype) if fmt != "cf32" else np.where(np.isfinite(raws[1]), raws[1] / 16, raws[1]).astype("<f4")
    ing = dab.Ingest(0, 3, fmt, rate, 0)
    models = [im.IngestModel(fmt, rate, 0) for _ in range(3)]
    run_rounds(ing, models, raws, rounds)
    assert all(m.g > 0 for m in models) and models[1].g != models[0].g
    ing.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rate", (2400000, 10000000))
@pytest.mark.parametrize("fmt", FORMATS)
def test_chunking_does_not_change_the_bytes(fmt, rate):
    rng = np.random.default_rng(rate // 1000 + 11 * len(fmt))
    sb = im.SAMPLE_BYTES[fmt]
    for gain, n in ((256, 20000), (0, W + 9000)):
        raws = [cases.random_raw(rng, fmt, n - 37 * b) for b in range(3)]
        one = dab.Ingest(0, 3, fmt, rate, gain)
        one.push(raws)
        want = [one.read(b) for b in range(3)]
        for b in range(3):
            assert np.array_equal(want[b], im.one_shot(fmt, rate, gain, raws[b])[0])
        gains = [one.gain(b) for b in range(3)]
        one.close()
        for on_device in (False, True):
            dev = []
            if on_device:
                for r in raws:
                    d = dab.DeviceBuffer(r.nbytes)
                    d.upload(r.view(np.uint8))
                    dev.append(d)
            ing = dab.Ingest(0, 3, fmt, rate, gain)
            cuts = [sorted([0, 0, len(r) // 2, len(r) // 2] + [int(v) for v in rng.integers(0, len(r) // 2 + 1, 9)]) for r in raws]
            got = [[] for _ in raws]
            for k in range(len(cuts[0]) - 1):
                if on_device:
                    ing.push_ptrs([dev[b].ptr + sb * cuts[b][k] for b in range(3)], [sb * (cuts[b][k + 1] - cuts[b][k]) for b in range(3)], on_device=True)
                else:
                    ing.push([raws[b][2 * cuts[b][k]:2 * cuts[b][k + 1]] for b in range(3)])
                for b in range(3):
                    got[b].append(ing.read(b))
            for b in range(3):
                assert np.array_equal(np.concatenate(got[b]), want[b]), (gain, on_device, b)
                assert ing.gain(b) == gains[b]
            ing.close()
            for d in dev:
                d.free()


@pytest.mark.gpu
def test_mixed_host_push_equals_one_device_push():
    """One host push of three streams of 0, 1 and 4097 samples (staging offsets 0, 0 and 16: the one sample's 4 bytes are rounded up) and a second one
    that completes them, against the same samples pushed from device memory in one piece.  Then the stage_ms entry's contract."""
    rng = np.random.default_rng(16)
    first = (0, 1, 4097)
    raws = [cases.random_raw(rng, "cs16", n + 3000 + 11 * b) for b, n in enumerate(first)]
    dev = [dab.DeviceBuffer(r.nbytes) for r in raws]
    for d, r in zip(dev, raws):
        d.upload(r.view(np.uint8))
    one = dab.Ingest(0, 3, "cs16", 2400000, 300)
    one.push_ptrs([d.ptr for d in dev], [r.nbytes for r in raws], on_device=True)
    want = [one.read(b) for b in range(3)]
    assert all(w.size > 2 * 2000 for w in want)
    one.close()
    ing = dab.Ingest(0, 3, "cs16", 2400000, 300)
    ing.push([r[:2 * n] for r, n in zip(raws, first)])
    got = [ing.read(b) for b in range(3)]
    ing.push([r[2 * n:] for r, n in zip(raws, first)])
    for b in range(3):
        assert np.array_equal(np.concatenate([got[b], ing.read(b)]), want[b]), b
    cases.check_stage_ms(ing, "dabhip_ingest_stage_ms", ("upload", "energy", "resample", "keep"))
    ing.close()
    for d in dev:
        d.free()


@pytest.mark.gpu
def test_push_refuses_part_of_a_sample():
    ing = dab.Ingest(0, 1, "cs16", 2400000, 256)
    with pytest.raises(dab.DabhipError, match="whole number"):
        ing.push([np.zeros(7, np.uint8)])
    with pytest.raises(dab.DabhipError, match="explicit gain"):
        dab.Ingest(0, 1, "cs16", 2400000, 0).skip(5)
    ing.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rate", (2400000, 10000000))
@pytest.mark.parametrize("fmt", ("cu8", "cs16"))
def test_positions_beyond_32_bits(fmt, rate):
    rng = np.random.default_rng(rate // 1000 + len(fmt))
    far = (1 << 32) + 12345
    raws = [cases.random_raw(rng, fmt, 5000 + b) for b in range(2)]
    ing = dab.Ingest(0, 2, fmt, rate, 300)
    models = [im.IngestModel(fmt, rate, 300) for _ in range(2)]
    run_rounds(ing, models, raws, [[40, 77]])
    ing.skip(far)
    for m in models:
        m.skip(far)
    assert all(ing.read(b).size == 0 for b in range(2))
    run_rounds(ing, models, [r[2 * 100:] for r in raws], [[3000, 2000], [1900, 2901]])
    ing.skip(3)                                   # fewer than T: they go through the filter
    for m in models:
        m.skip(3)
    run_rounds(ing, models, raws, [[500, 1]])
    assert models[0].pushed > far + 4900
    ing.close()


@pytest.fixture(scope="module")
def capture_cs16():
    """The CPU test's 2.4 Msps cs16 capture, the model's cu8 of it and the oracle's frames of that."""
    raw = cases.raw(0, "cs16")
    out, _ = cases.model_output(0, "cs16")
    eti, _ = ol.or_replay(out)
    assert len(eti) > 0
    return raw, out, eti


@pytest.mark.gpu
def test_through_the_decoder(capture_cs16):
    raw, out, want = capture_cs16
    ing = dab.Ingest(0, 1, "cs16", cases.RATE, 256)
    ing.push([raw])
    assert np.array_equal(ing.read(0), out)
    eng = dab.Engine(0)
    ptrs, sizes = ing.output_ptrs()
    assert eng.decode_device(ptrs, sizes) == len(want)
    assert np.array_equal(eng.eti(0), want)
    eng.close()
    ing.close()


@pytest.mark.gpu
def test_through_a_session_in_odd_segments(capture_cs16):
    raw, out, want = capture_cs16
    n = raw.size // 2
    ing = dab.Ingest(0, 1, "cs16", cases.RATE, 256)
    ses = dab.Stream(1)
    frames, at = [], 0
    for k, step in enumerate([333333, 1, 777777, 0, 1234567, 99999] + [1000003] * 8):
        step = min(step, n - at)
        ing.push([raw[2 * at:2 * (at + step)]])
        ptrs, sizes = ing.output_ptrs()
        ses.feed_ptrs(ptrs, sizes, on_device=True)
        frames.append(ses.eti(0))
        at += step
    assert at == n
    assert np.array_equal(np.concatenate(frames), want)
    ses.close()
    ing.close()


@pytest.mark.gpu
def test_identity_through_the_decoder():
    iq = cases.direct(0)
    eng = dab.Engine(0)
    assert eng.decode([iq]) > 0
    want = eng.eti(0)
    ing = dab.Ingest(0, 1, "cu8", 2048000, 256)
    ing.push([iq])
    assert np.array_equal(ing.read(0), iq)
    ptrs, sizes = ing.output_ptrs()
    assert eng.decode_device(ptrs, sizes) == len(want)
    assert np.array_equal(eng.eti(0), want)
    eng.close()
    ing.close()


@pytest.mark.gpu
def test_cli(tmp_path, capture_cs16):
    raw, _, _ = capture_cs16
    # the API path with the CLI's default, the automatic gain
    ing = dab.Ingest(0, 1, "cs16", cases.RATE, 0)
    ing.push([raw])
    eng = dab.Engine(0)
    ptrs, sizes = ing.output_ptrs()
    assert eng.decode_device(ptrs, sizes) > 0
    want = eng.eti(0).tobytes()
    eng.close()
    ing.close()
    path = tmp_path / "capture.cs16"
    raw.tofile(path)
    run = subprocess.run([CLI, "--quiet", "--format", "cs16", "--rate", str(cases.RATE), str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == want
    # the same on stdin, written in pieces that end inside samples, and three stray bytes at the very end
    data = raw.tobytes() + b"\x01\x02\x03"
    proc = subprocess.Popen([CLI, "--quiet", "--stream", "--segment-calls", "3", "--format", "cs16", "--rate", str(cases.RATE), "-"], stdin=subprocess.PIPE,
                            stdout=open(tmp_path / "out.eti", "wb"), stderr=subprocess.PIPE)
    for at in range(0, len(data), 1000003):
        proc.stdin.write(data[at:at + 1000003])
        proc.stdin.flush()
    proc.stdin.close()
    err = proc.stderr.read()
    assert proc.wait(timeout=120) == 0, err[-2000:]
    assert open(tmp_path / "out.eti", "rb").read() == want


def test_cli_refuses_ingest_on_two_devices(tmp_path):
    path = tmp_path / "capture.cs16"
    path.write_bytes(b"\0" * 64)
    run = subprocess.run([CLI, "--format", "cs16", "--rate", "2400000", "--devices", "0,1", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert run.returncode == 1 and run.stdout == b""
    assert b"one device" in run.stderr
