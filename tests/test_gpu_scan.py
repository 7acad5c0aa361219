"""The block scan on the GPU (include/dabhip.h, "block scan"; csrc/k_scan.hip, csrc/scan.cpp): the spectrum against the numpy model
(tests/scan_model.py) bit for bit -- every format, stream lengths around one segment, one and two workgroups per stream, the window's end inside a
push, full-scale input, random chunkings from host and device memory --, the blocks against the model's rule, the offsets found through the tuned
ingest and the decoder, and the CLI's --scan and --tune auto."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import dabtools_amd as dab
import ingest_cases as cases
import ingest_model as im
import scan_cases as sc
import scan_model as sm
import tune_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dabtools_amd", "dab2eti-hip")
FORMATS = ("cu8", "cs8", "cs16", "cf32")
RATES = (2048000, 4096000, 10000000)
S, G = sm.S, 8                                                    # a segment, and the segments one workgroup sums (k_scan.hip: kScanGroup)


def check(scan, models):
    for b, m in enumerate(models):
        P, done = scan.spectrum(b)
        assert done == m.done, (b, done, m.done)
        assert np.array_equal(P, m.P), (b, int(np.flatnonzero(P != m.P)[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_bit_exact_against_the_model(fmt, rate):
    """Five streams at once: no sample, 4095 samples (no segment: an all-zero spectrum), exactly one segment, G segments (one workgroup) and G + 1 and
    a bit (two workgroups add into one P).  Then one more sample each: the 4095 become a segment."""
    rng = np.random.default_rng(rate // 1000 + 7 * len(fmt))
    lengths = [0, S - 1, S, G * S, (G + 1) * S + 100]
    raws = [cases.random_raw(rng, fmt, n + 1) for n in lengths]
    scan = dab.Scan(0, len(lengths), fmt, rate)
    models = [sm.ScanModel(fmt) for _ in lengths]
    first = [r[:2 * n] for r, n in zip(raws, lengths)]
    assert scan.push(first) == sum(m.push(p) for m, p in zip(models, first)) == 0 + 0 + 1 + G + G + 1
    check(scan, models)
    assert not scan.spectrum(0)[0].any() and not scan.spectrum(1)[0].any() and scan.spectrum(2)[0].any()
    assert scan.push([r[-2:] for r in raws]) == sum(m.push(r[-2:]) for m, r in zip(models, raws)) == 1
    check(scan, models)
    assert set(scan.stage_ms()) == {"upload", "transform", "keep"}
    scan.close()


@pytest.mark.gpu
def test_the_window_ends_inside_a_push():
    rng = np.random.default_rng(3)
    raws = [cases.random_raw(rng, "cs16", 9 * S) for _ in range(2)]
    scan = dab.Scan(0, 2, "cs16", 4096000, 3)
    models = [sm.ScanModel("cs16", 3) for _ in range(2)]
    # stream 0: 2.5 segments, then 4 more (the third completes, the rest is past the window); stream 1: everything at once
    for parts, want in (([raws[0][:5 * S], raws[1]], 2 + 3), ([raws[0][5 * S:13 * S], raws[1][:0]], 1), ([raws[0][13 * S:], raws[1]], 0)):
        assert scan.push(parts) == sum(m.push(p) for m, p in zip(models, parts)) == want
        check(scan, models)
    for b in range(2):
        assert np.array_equal(scan.spectrum(b)[0], sm.spectrum("cs16", raws[b][:2 * 3 * S], 3)[0])
    scan.close()


def full_scale_segments(fmt):
    """Both rails at the format's extremes: constant, alternating, turning at 45 degrees, square waves, random signs."""
    lo, hi = (0, 255) if fmt == "cu8" else (-32768, 32767)
    n = np.arange(S)
    rng = np.random.default_rng(5)
    rails = [np.full(S, hi), np.full(S, lo), np.where(n % 2 == 0, hi, lo), np.where(n % 2 == 0, lo, hi)]
    rails += [np.where(np.cos(2 * np.pi * k0 * n / S + 0.1) >= 0, hi, lo) for k0 in (1, 2, 300, 1024)]
    rails += [np.where(rng.integers(0, 2, S) == 1, hi, lo) for _ in range(4)]
    segs = [np.stack([a, b], axis=1) for a in rails[:4] for b in rails[:4]] + [np.stack([a, a], axis=1) for a in rails[4:]] + [np.stack([rails[6], rails[7]], axis=1)]
    mid, amp = (127.0, 128.0 * np.sqrt(2)) if fmt == "cu8" else (0.0, 32768.0 * np.sqrt(2))
    for k0 in (1, 511, 512, 1024, 1537, 3000):
        ph = 2 * np.pi * (k0 * n / S + 1 / 8)
        segs.append(np.clip(np.rint(mid + amp * np.stack([np.cos(ph), np.sin(ph)], axis=1)), lo, hi))
    return np.array(segs).astype(im.DTYPES[fmt]).reshape(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ("cu8", "cs16"))
def test_full_scale_input(fmt):
    """The header's int32 claim: full-scale input whose energy gathers in single bins (cu8's 255 is +32768, cs16 reaches -32768)."""
    raw = full_scale_segments(fmt)
    want, done = sm.spectrum(fmt, raw, 64)
    assert done == raw.size // (2 * S) > 2 * G and int(want.max()) > (46000 ** 2 // 2)
    scan = dab.Scan(0, 1, fmt, 8000000)
    assert scan.push([raw]) == done
    assert np.array_equal(scan.spectrum(0)[0], want)
    scan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("on_device", (False, True))
@pytest.mark.parametrize("fmt", FORMATS)
def test_chunking_does_not_change_the_spectrum(fmt, on_device):
    rng = np.random.default_rng(11 * len(fmt) + on_device)
    sb = im.SAMPLE_BYTES[fmt]
    n = 11 * S + 77
    raws = [cases.random_raw(rng, fmt, n - 1000 * b) for b in range(2)]
    want = [sm.spectrum(fmt, r, 10) for r in raws]                # the window ends before the streams do
    # pushes of 1 sample and of 4097, empty ones, cuts at and around a segment's end, random cuts
    cuts = [sorted([0, 0, 1, 2, S - 1, S, S + 4097, S + 4098, 3 * S + 1, len(r) // 2, len(r) // 2] + [int(v) for v in rng.integers(0, len(r) // 2 + 1, 6)]) for r in raws]
    dev = []
    if on_device:                                                 # one sample into the allocation: aligned to a sample and to nothing more
        for r in raws:
            d = dab.DeviceBuffer(r.nbytes + sb)
            d.upload(np.concatenate([np.zeros(sb, np.uint8), r.view(np.uint8)]))
            dev.append(d)
    scan = dab.Scan(0, 2, fmt, 4096000, 10)
    for k in range(len(cuts[0]) - 1):
        if on_device:
            scan.push_ptrs([dev[b].ptr + sb * (1 + cuts[b][k]) for b in range(2)], [sb * (cuts[b][k + 1] - cuts[b][k]) for b in range(2)], on_device=True)
        else:
            scan.push([raws[b][2 * cuts[b][k]:2 * cuts[b][k + 1]] for b in range(2)])
    for b in range(2):
        P, done = scan.spectrum(b)
        assert done == want[b][1] == 10 and np.array_equal(P, want[b][0]), (b, on_device)
    scan.close()
    for d in dev:
        d.free()


@pytest.mark.gpu
def test_mixed_host_push_equals_one_device_push():
    """One host push of three streams of 0, 1 and 4097 samples and a second one that runs past the window of 2 segments (the host path uploads only
    what the window still lacks), against the same samples pushed from device memory in one piece.  Then the stage_ms entry's contract."""
    rng = np.random.default_rng(16)
    first = (0, 1, 4097)
    raws = [cases.random_raw(rng, "cs16", 2 * S + 500 + 11 * b) for b in range(3)]
    dev = [dab.DeviceBuffer(r.nbytes) for r in raws]
    for d, r in zip(dev, raws):
        d.upload(r.view(np.uint8))
    one = dab.Scan(0, 3, "cs16", 4096000, 2)
    assert one.push_ptrs([d.ptr for d in dev], [r.nbytes for r in raws], on_device=True) == 6
    want = [one.spectrum(b) for b in range(3)]
    one.close()
    scan = dab.Scan(0, 3, "cs16", 4096000, 2)
    assert scan.push([r[:2 * n] for r, n in zip(raws, first)]) == 1
    assert scan.push([r[2 * n:] for r, n in zip(raws, first)]) == 5
    assert scan.push(raws) == 0                                   # the window is done: nothing is uploaded
    for b in range(3):
        P, done = scan.spectrum(b)
        assert done == want[b][1] == 2 and P.any() and np.array_equal(P, want[b][0]), b
    cases.check_stage_ms(scan, "dabhip_scan_stage_ms", ("upload", "transform", "keep"))
    scan.close()
    for d in dev:
        d.free()


@pytest.mark.gpu
def test_refusals_of_push():
    scan = dab.Scan(0, 1, "cs16", 4096000)
    with pytest.raises(dab.DabhipError, match="no whole number"):
        scan.push([np.zeros(6, np.uint8)])
    d = dab.DeviceBuffer(64)
    with pytest.raises(dab.DabhipError, match="aligned to its sample size"):
        scan.push_ptrs([d.ptr + 2], [8], on_device=True)
    with pytest.raises(dab.DabhipError, match="bad argument"):
        scan.spectrum(1)
    d.free()
    scan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(tc.VARIANTS))
def test_blocks_against_the_models_rule(variant):
    """The whole 20 TF capture pushed: the window is its first 64 segments, which are scan_cases' capture of the same name."""
    fmt = tc.VARIANTS[variant][0]
    scan = dab.Scan(0, 1, fmt, tc.RATE)
    assert scan.push([tc.raw(variant)]) == 64
    P, done = scan.spectrum(0)
    want, _ = sc.model_spectrum(variant)
    assert done == 64 and np.array_equal(P, want)
    for center in (0, sc.CENTER):
        assert scan.blocks(0, center) == dab.scan_detect(want, tc.RATE, center) == sm.detect(want, tc.RATE, center)
    assert [r["name"] for r in scan.blocks(0, sc.CENTER)] == ["5A", "5B"]
    scan.close()


def decode_tuned(raw, fmt, offsets):
    ing = dab.Ingest(0, 1, fmt, tc.RATE, 0, offsets=offsets)
    ing.push([raw])
    eng = dab.Engine(0)
    ptrs, sizes = ing.output_ptrs()
    total = eng.decode_device(ptrs, sizes)
    eti = [eng.eti(c) for c in range(len(offsets))]
    eng.close()
    ing.close()
    return total, eti


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(tc.VARIANTS))
def test_scan_then_tune_then_decode(variant):
    fmt, raw = tc.VARIANTS[variant][0], tc.raw(variant)
    scan = dab.Scan(0, 1, fmt, tc.RATE)
    scan.push([raw])
    found = [r["offset_hz"] for r in scan.blocks(0, sc.CENTER)]
    scan.close()
    assert found == list(tc.OFFSETS)
    total, eti = decode_tuned(raw, fmt, found)
    want_total, want = decode_tuned(raw, fmt, tc.OFFSETS)
    assert total == want_total > 0 and all(len(w) > 0 for w in want)
    for c in range(2):
        assert np.array_equal(eti[c], want[c])


def run_cli(args, timeout=120, **kw):
    return subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, **kw)


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    path = tmp_path_factory.mktemp("scan") / "capture.cs16"
    tc.raw("cs16_plus20").tofile(path)
    return path


LINE = re.compile(r"^(.*): offset (-?\d+) Hz, block (\S+), width (\d+) Hz, level (-?[\d.]+) dBFS, contrast (-?[\d.]+) dB$")


def check_lines(text, name, center, P=None):
    want = sm.detect(sc.model_spectrum("cs16_plus20")[0] if P is None else P, tc.RATE, center)
    lines = text.decode().splitlines()
    assert len(lines) == len(want) == 2
    for line, r in zip(lines, want):
        m = LINE.match(line)
        assert m, line
        assert (m.group(1), int(m.group(2)), m.group(3), int(m.group(4))) == (name, r["offset_hz"], r["name"] or "-", r["width_hz"])
        mean_in = r["in"] / r["nin"]
        level = 10 * math.log10(mean_in / 64 * (1536000 * S / tc.RATE) / 32768.0 ** 2)
        contrast = 10 * math.log10(mean_in / (max(r["lo"], r["hi"]) / r["ng"]))
        assert abs(float(m.group(5)) - level) < 0.06 and abs(float(m.group(6)) - contrast) < 0.06
    return want


@pytest.mark.gpu
def test_cli_scan(capture):
    base = ["--format", "cs16", "--rate", str(tc.RATE), "--scan"]
    run = run_cli(base + [str(capture)])
    assert run.returncode == 0, run.stderr[-2000:]
    recs = check_lines(run.stdout, str(capture), 0)
    # block 1 is 8000 LSB rms per rail, 20 dB above block 0: -9.2 dB below a full-scale tone, and the strong block's guards hold nothing
    lines = [LINE.match(l) for l in run.stdout.decode().splitlines()]
    assert abs(float(lines[1].group(5)) - 10 * math.log10(2 * 8000.0 ** 2 / 32768.0 ** 2)) < 0.5 and abs(float(lines[1].group(5)) - float(lines[0].group(5)) - 20.0) < 0.5
    assert [r["name"] for r in recs] == ["", ""]
    run = run_cli(base + ["--center", str(sc.CENTER), "-"], input=tc.raw("cs16_plus20").tobytes()[:3000001])      # a pipe that ends inside a sample
    assert run.returncode == 0, run.stderr[-2000:]
    assert [r["name"] for r in check_lines(run.stdout, "-", sc.CENTER)] == ["5A", "5B"]


@pytest.mark.gpu
def test_cli_tune_auto(capture):
    data = tc.raw("cs16_plus20").tobytes()
    base = ["--quiet", "--format", "cs16", "--rate", str(tc.RATE)]
    auto = ["--tune", "auto", "--center", str(sc.CENTER)]
    explicit = ["--tune", ",".join(str(f) for f in tc.OFFSETS)]
    want = run_cli(base + explicit + [str(capture)])
    assert want.returncode == 0 and len(want.stdout) > 2 * 6144, want.stderr[-2000:]
    got = run_cli(base + auto + [str(capture)])
    assert got.returncode == 0, got.stderr[-2000:]
    assert got.stdout == want.stdout
    assert b"capture.cs16@-856000: " in got.stderr and b"capture.cs16@856000: " in got.stderr
    # a pipe: the scanned samples are kept and go through the ingest stage first
    piped = ["--stream", "--segment-calls", "3"]
    want = run_cli(base + piped + explicit + ["-"], input=data)
    got = run_cli(base + piped + auto + ["-"], input=data)
    assert want.returncode == 0 and got.returncode == 0, (want.stderr[-1000:], got.stderr[-1000:])
    assert len(want.stdout) > 2 * 6144 and got.stdout == want.stdout


@pytest.mark.gpu
def test_cli_tune_auto_without_a_centre(tmp_path):
    """The offsets are measured: the weak block is tuned 1.5 kHz off and the software AFC pulls it in, which takes some 7 TF, and frames leave 15 TF
    later: a capture of 32 TF (the CPU oracle with the reference's tuner rule gives 44 frames of the weak block and 60 of the strong one)."""
    raw = sc.long_raw()
    path = tmp_path / "capture.cs16"
    raw.tofile(path)
    P, _ = sm.spectrum("cs16", raw[:2 * 64 * S], 64)
    run = run_cli(["--format", "cs16", "--rate", str(tc.RATE), "--tune", "auto", "--afc", str(path)])
    assert run.returncode == 0, run.stderr[-2000:]
    err = run.stderr.decode()
    found = check_lines("\n".join(l for l in err.splitlines() if LINE.match(l)).encode(), str(path), 0, P)      # the scan lines, on stderr
    counts = re.findall(r"capture\.cs16@(-?\d+): (\d+) ETI frames", err)
    assert [int(f) for f, _ in counts] == [r["offset_hz"] for r in found] and all(abs(int(f) - o) <= 2000 for (f, _), o in zip(counts, tc.OFFSETS))
    assert int(counts[0][0]) != tc.OFFSETS[0]                     # the weak block is off the raster: it is the AFC that brings it in
    assert all(int(n) >= 16 for _, n in counts) and len(run.stdout) == 6144 * sum(int(n) for _, n in counts)
    assert "Locked" in err and "--afc is recommended" not in err


@pytest.mark.parametrize("args, code, text", [
    (["--scan"], 1, b"--scan needs --rate"),
    (["--tune", "auto"], 1, b"--tune auto needs --rate"),
    (["--rate", "4096000", "--center", "175784000"], 1, b"--center goes with --scan or --tune auto"),
    (["--rate", "4096000", "--tune", "856000", "--center", "175784000"], 1, b"--center goes with --scan or --tune auto"),
    (["--rate", "4096000", "--scan", "--tune", "856000"], 1, b"does not go with --tune"),
    (["--rate", "4096000", "--scan", "--tune", "auto"], 1, b"does not go with --tune"),
    (["--rate", "4096000", "--scan", "--center", "0"], 1, b"--center takes"),
    (["--rate", "4096000", "--scan", "--devices", "0,1"], 1, b"one device"),
    (["--rate", "12000000", "--scan"], 2, b"outside 2048000 .. 10240000"),
])
def test_cli_refusals(tmp_path, args, code, text):
    path = tmp_path / "capture.cs16"
    path.write_bytes(b"\0" * 64)
    run = run_cli(["--format", "cs16"] + args + [str(path)], timeout=60)
    assert run.returncode == code and run.stdout == b""
    assert text in run.stderr


@pytest.mark.gpu
def test_cli_nothing_found_and_unequal_counts(tmp_path, capture):
    empty, one = tmp_path / "empty.cs16", tmp_path / "one.cs16"
    empty.write_bytes(b"\0" * (4 * 70 * S))
    sc.raw("cs16_plus26").tofile(one)                             # only the strong block is found in it
    base = ["--format", "cs16", "--rate", str(tc.RATE)]
    run = run_cli(base + ["--scan", str(empty), str(one)])
    assert run.returncode == 0 and run.stdout.decode().splitlines()[0] == "%s: no DAB block found" % empty
    assert len(run.stdout.decode().splitlines()) == 2 and LINE.match(run.stdout.decode().splitlines()[1]).group(1) == str(one)
    run = run_cli(base + ["--tune", "auto", str(capture), str(empty)])
    assert run.returncode == 1 and run.stdout == b"" and ("no DAB block found in %s" % empty).encode() in run.stderr
    run = run_cli(base + ["--tune", "auto", str(capture), str(one)])
    assert run.returncode == 1 and run.stdout == b"" and b"must hold the same number" in run.stderr and b"--afc is recommended" not in run.stderr
    run = run_cli(base + ["--tune", "auto", str(one)])            # no --center and no --afc: the recommendation
    assert run.returncode == 0 and b"--afc is recommended" in run.stderr and b"one.cs16@856000: " in run.stderr
