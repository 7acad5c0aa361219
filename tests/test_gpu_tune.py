"""The ingest stage's tuned mode on the GPU (include/dabhip.h, "ingest stage, tuned mode"; csrc/k_ingest.hip, csrc/ingest.cpp): its bytes against
the numpy model (tests/tune_model.py) for every format and ratio class, across pushes, with the NCO phase and the positions wrapping at 2^32, the
automatic gain per channel, through the decoder and through the CLI."""
import os
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import ingest_cases as cases
import ingest_model as im
import oracle_lib as ol
import tune_cases as tc
import tune_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dabtools_amd", "dab2eti-hip")
FORMATS = ("cu8", "cs8", "cs16", "cf32")
RATES = (2048000, 2400000, 4096000, 10000000)                         # 1/1 (the mixer alone), 64/75, 1/2, 128/625 (the table beyond 64 KiB of LDS)
TILE, GROUP = 1024, 8 * 1024                                          # outputs of one tile, and of the tiles one workgroup walks (k_ingest.hip)
W = im.W


def offsets_of(rate):
    """A negative, the zero and a positive offset: the lowest block the capture holds, its centre, and an odd number of Hz."""
    reach = rate // 2 - 768000
    return [-reach, 0, reach * 2 // 3 + 1]


def run_rounds(ing, models, raws, rounds):
    """models[b][c]: channel c of stream b.  rounds: per round the samples each stream pushes.  Every round's bytes and gains against the models'."""
    nch = len(models[0])
    at = [0] * len(models)
    for sizes in rounds:
        parts = [raws[b][2 * at[b]:2 * (at[b] + n)] for b, n in enumerate(sizes)]
        total = ing.push(parts)
        want = [[m.push(p) for m in ms] for ms, p in zip(models, parts)]
        assert total == sum(w.size for ws in want for w in ws)
        for b, ws in enumerate(want):
            for c, w in enumerate(ws):
                got = ing.read(b * nch + c)
                assert got.size == w.size, (b, c, sizes, got.size, w.size)
                assert np.array_equal(got, w), (b, c, sizes, int(np.flatnonzero(got != w)[0]))
                assert ing.gain(b * nch + c) == models[b][c].g
        at = [a + n for a, n in zip(at, sizes)]


@pytest.mark.gpu
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_bit_exact_against_the_model(fmt, rate):
    rng = np.random.default_rng(rate // 1000 + 7 * len(fmt))
    _, L, M, T = dab.ingest_tune_taps(fmt, rate)
    offsets = offsets_of(rate)
    # two streams of different lengths, three channels each.  First the first output's edge (T/2 samples: nothing; one more: output 0) and a few
    # thousand samples; then stream 0 up to a workgroup's 8 tiles, one output and one more tile and a bit (9300 outputs), stream 1 to 8 tiles + 1
    h = T // 2
    rounds = [[h, 3001], [1, 0]]
    done = [h + 1, 3001]
    last = [cases.samples_for_outputs(L, M, T, GROUP + 1 + TILE + 83) - done[0], cases.samples_for_outputs(L, M, T, GROUP + 1) - done[1]]
    rounds.append(last)
    raws = [cases.random_raw(rng, fmt, done[b] + last[b]) for b in range(2)]
    ing = dab.Ingest(0, 2, fmt, rate, 300, offsets=offsets)
    assert (ing.nchannels, ing.nouts, len(ing.output_ptrs()[0])) == (3, 6, 6)
    models = [[tm.TuneModel(fmt, rate, f, 300) for f in offsets] for _ in range(2)]
    run_rounds(ing, models, raws, rounds)
    assert models[0][0].produced == GROUP + 1 + TILE + 83 and models[1][2].produced == GROUP + 1
    if fmt != "cf32":                                             # full-range input: the mixer's clamp is hit in both directions
        y = models[0][2].x
        assert (y == 32767).any() and (y == -32768).any()
    assert set(ing.stage_ms()) == {"upload", "energy", "resample", "keep"}
    ing.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rate", (2400000, 10000000))
@pytest.mark.parametrize("fmt", FORMATS)
def test_chunking_does_not_change_the_bytes(fmt, rate):
    rng = np.random.default_rng(rate // 1000 + 11 * len(fmt))
    sb = im.SAMPLE_BYTES[fmt]
    T = dab.ingest_tune_taps(fmt, rate)[3]
    offsets = offsets_of(rate)[::2]
    n = 12000
    raws = [cases.random_raw(rng, fmt, n - 37 * b) for b in range(2)]
    want = [[out for out, _ in tm.one_shot(fmt, rate, 256, r, offsets)] for r in raws]
    one = dab.Ingest(0, 2, fmt, rate, 256, offsets=offsets)
    one.push(raws)
    for b in range(2):
        for c in range(2):
            assert np.array_equal(one.read(2 * b + c), want[b][c])
    one.close()
    for on_device in (False, True):
        dev = []
        if on_device:
            for r in raws:
                d = dab.DeviceBuffer(r.nbytes)
                d.upload(r.view(np.uint8))
                dev.append(d)
        ing = dab.Ingest(0, 2, fmt, rate, 256, offsets=offsets)
        # empty and one-sample pushes, pushes that end on the first output's edge (T/2 samples: none yet, T/2 + 1: output 0), random cuts
        cuts = [sorted([0, 0, 1, T // 2, T // 2 + 1, len(r) // 2, len(r) // 2] + [int(v) for v in rng.integers(0, len(r) // 2 + 1, 7)]) for r in raws]
        got = [[] for _ in range(4)]
        for k in range(len(cuts[0]) - 1):
            if on_device:
                ing.push_ptrs([dev[b].ptr + sb * cuts[b][k] for b in range(2)], [sb * (cuts[b][k + 1] - cuts[b][k]) for b in range(2)], on_device=True)
            else:
                ing.push([raws[b][2 * cuts[b][k]:2 * cuts[b][k + 1]] for b in range(2)])
            for o in range(4):
                got[o].append(ing.read(o))
        for o in range(4):
            assert np.array_equal(np.concatenate(got[o]), want[o // 2][o % 2]), (on_device, o)
        ing.close()
        for d in dev:
            d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("rate", (2048000, 2400000, 10000000))
@pytest.mark.parametrize("fmt", ("cu8", "cs16"))
def test_phase_and_positions_wrap_at_32_bits(fmt, rate):
    rng = np.random.default_rng(rate // 1000 + len(fmt))
    offsets = offsets_of(rate)[::2]
    raws = [cases.random_raw(rng, fmt, 6000 + b) for b in range(2)]
    ing = dab.Ingest(0, 2, fmt, rate, 300, offsets=offsets)
    models = [[tm.TuneModel(fmt, rate, f, 300) for f in offsets] for _ in range(2)]
    run_rounds(ing, models, raws, [[40, 77]])
    below = (1 << 32) - 1500                      # the pushes after it cross 2^32: the positions' low words and n step mod 2^32 both wrap
    ing.skip(below)
    for m in sum(models, []):
        m.skip(below)
    assert all(ing.read(o).size == 0 for o in range(4))
    run_rounds(ing, models, [r[2 * 100:] for r in raws], [[1400, 1300], [1600, 1801]])
    assert models[0][0].pushed > 1 << 32 and (1 << 32) - 200 < below + 77 + 1300 < 1 << 32
    ing.skip(3)                                   # fewer than T: they go through the filter
    ing.skip(1 << 32)                             # and once more round, to beyond 2^33
    for m in sum(models, []):
        m.skip(3)
        m.skip(1 << 32)
    run_rounds(ing, models, raws, [[2500, 1]])
    assert models[0][0].pushed > (1 << 33)
    ing.close()


@pytest.mark.gpu
def test_index_rounding_wraps_to_entry_zero():
    """Offsets of -1 and -100 Hz: theta stays within 2^19 of a full turn for the first 292 (2) samples, where i computes to 4096 and must be 0."""
    rate, offsets = 2400000, [-1, -100, 431999]
    for f, visits in zip(offsets[:2], (292, 2)):
        theta = (np.arange(1, 3000, dtype=np.uint64) * np.uint64(tm.step_rule(rate, f))) & np.uint64(tm.M32)
        assert int((theta[:300] >= (1 << 32) - (1 << 19)).sum()) == visits
    rng = np.random.default_rng(4)
    raws = [cases.random_raw(rng, "cs16", 3000)]
    ing = dab.Ingest(0, 1, "cs16", rate, 256, offsets=offsets)
    run_rounds(ing, [[tm.TuneModel("cs16", rate, f, 256) for f in offsets]], raws, [[1500], [1500]])
    ing.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rate", (2048000, 4096000))
def test_automatic_gain_per_channel(rate):
    """A strong carrier-like block at +f and one 40 dB below it at -f: each channel measures its own first W outputs.  Stream 0's window closes
    inside a push, stream 1's exactly at a push's end; gain() is 0 until then (run_rounds compares it with the model's after every push)."""
    rng = np.random.default_rng(rate // 1000)
    _, L, M, T = dab.ingest_tune_taps("cs16", rate)
    f = rate // 2 - 768000 if rate == 2048000 else 856000
    closes_at = cases.samples_for_outputs(L, M, T, W)
    rounds = [[closes_at - 100, closes_at - 100], [3000, 100], [0, 2900]]
    raws = []
    for b in range(2):
        n = sum(r[b] for r in rounds)
        t = np.arange(n) * (2 * np.pi * f / rate)
        x = 8000.0 * np.exp(1j * t) + 80.0 * np.exp(-1j * t) + (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (2.0 + b)
        raws.append(np.rint(np.stack([x.real, x.imag], axis=1)).reshape(-1).astype("<i2"))
    ing = dab.Ingest(0, 2, "cs16", rate, 0, offsets=[-f, f])
    models = [[tm.TuneModel("cs16", rate, o, 0) for o in (-f, f)] for _ in range(2)]
    run_rounds(ing, models, raws, rounds[:1])
    assert [ing.gain(o) for o in range(4)] == [0, 0, 0, 0] and all(ing.read(o).size == 0 for o in range(4))
    run_rounds(ing, models, [r[2 * rounds[0][b]:] for b, r in enumerate(raws)], rounds[1:])
    for ms in models:
        assert ms[0].g > 0 and ms[1].g > 0
        if T:                                                     # (without a filter both channels hold both carriers)
            assert ms[0].g > 50 * ms[1].g                         # 40 dB apart in level: the gains a factor of about 100
    ing.close()


@pytest.fixture(scope="module")
def two_blocks():
    """The CPU test's capture with the second block 20 dB stronger (cs16 at 4.096 Msps), the model's cu8 of both channels and the oracle's frames."""
    raw = tc.raw("cs16_plus20")
    outs = [tc.model_output("cs16_plus20", c)[0] for c in range(2)]
    etis = [ol.or_replay(o)[0] for o in outs]
    assert all(len(e) > 0 for e in etis)
    return raw, outs, etis


@pytest.mark.gpu
def test_through_the_decoder(two_blocks):
    raw, outs, want = two_blocks
    ing = dab.Ingest(0, 1, "cs16", tc.RATE, 0, offsets=tc.OFFSETS)
    ing.push([raw])
    for c in range(2):
        assert np.array_equal(ing.read(c), outs[c])
    eng = dab.Engine(0)
    ptrs, sizes = ing.output_ptrs()
    assert eng.decode_device(ptrs, sizes) == sum(len(w) for w in want)
    for c in range(2):
        assert np.array_equal(eng.eti(c), want[c])
    eng.close()
    ing.close()


@pytest.mark.gpu
def test_through_a_session_in_odd_segments(two_blocks):
    raw, outs, want = two_blocks
    n = raw.size // 2
    ing = dab.Ingest(0, 1, "cs16", tc.RATE, 0, offsets=tc.OFFSETS)
    ses = dab.Stream(2)
    frames, at = [[], []], 0
    for step in [33333, 1, 777777, 0, 1234567, 99999] + [1000003] * 8:
        step = min(step, n - at)
        ing.push([raw[2 * at:2 * (at + step)]])
        ptrs, sizes = ing.output_ptrs()
        ses.feed_ptrs(ptrs, sizes, on_device=True)
        for c in range(2):
            frames[c].append(ses.eti(c))
        at += step
    assert at == n
    for c in range(2):
        assert np.array_equal(np.concatenate(frames[c]), want[c])
    ses.close()
    ing.close()


@pytest.mark.gpu
def test_cli(tmp_path, two_blocks):
    raw, _, _ = two_blocks
    ing = dab.Ingest(0, 1, "cs16", tc.RATE, 0, offsets=tc.OFFSETS)
    ing.push([raw])
    eng = dab.Engine(0)
    ptrs, sizes = ing.output_ptrs()
    assert eng.decode_device(ptrs, sizes) > 0
    want = [eng.eti(c).tobytes() for c in range(2)]
    eng.close()
    ing.close()
    assert len(want[0]) > 0 and len(want[1]) > 0
    path = tmp_path / "capture.cs16"
    raw.tofile(path)
    tune = ",".join(str(f) for f in tc.OFFSETS)
    run = subprocess.run([CLI, "--quiet", "--format", "cs16", "--rate", str(tc.RATE), "--tune", tune, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stdout == want[0] + want[1]                        # block after block, as the frames of two files
    assert b"capture.cs16@-856000: " in run.stderr and b"capture.cs16@856000: " in run.stderr
    # the same on stdin, written in pieces that end inside samples, and three stray bytes at the very end: the blocks' frames leave segment by
    # segment, each block's in order (the two ensembles' frames differ, so every frame says whose it is)
    data = raw.tobytes() + b"\x01\x02\x03"
    proc = subprocess.Popen([CLI, "--quiet", "--stream", "--segment-calls", "3", "--format", "cs16", "--rate", str(tc.RATE), "--tune", tune, "-"], stdin=subprocess.PIPE,
                            stdout=open(tmp_path / "out.eti", "wb"), stderr=subprocess.PIPE)
    for at in range(0, len(data), 1000003):
        proc.stdin.write(data[at:at + 1000003])
        proc.stdin.flush()
    proc.stdin.close()
    err = proc.stderr.read()
    assert proc.wait(timeout=120) == 0, err[-2000:]
    got = open(tmp_path / "out.eti", "rb").read()
    assert len(got) == len(want[0]) + len(want[1])
    owner = [{w[k:k + 6144] for k in range(0, len(w), 6144)} for w in want]
    assert not owner[0] & owner[1]
    split = [b"", b""]
    for k in range(0, len(got), 6144):
        f = got[k:k + 6144]
        assert (f in owner[0]) != (f in owner[1])
        split[f in owner[1]] += f
    assert split == want


@pytest.mark.parametrize("args, code, text", [
    (["--tune", "856000"], 1, b"needs --rate"),
    (["--rate", "4096000", "--tune", "856000,"], 1, b"HZ[,HZ...]"),
    (["--rate", "4096000", "--tune", "85x"], 1, b"HZ[,HZ...]"),
    (["--rate", "4096000", "--tune", "856000", "--devices", "0,1"], 1, b"one device"),
    (["--rate", "4096000", "--tune", "1280001"], 2, b"do not lie within"),
    (["--rate", "4096000", "--tune", ",".join(["0"] * 17)], 2, b"nchannels must be 1 .. 16"),
])
def test_cli_refusals(tmp_path, args, code, text):
    path = tmp_path / "capture.cs16"
    path.write_bytes(b"\0" * 64)
    run = subprocess.run([CLI, "--format", "cs16"] + args + [str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert run.returncode == code and run.stdout == b""
    assert text in run.stderr
