"""GPU parity tests, third batch: a randomised sweep against the oracle inside the suite, and BASELINE configs[2] on exactly the
workload bench.py times (256 DISTINCT device-modulated ensembles x 64 TF)."""
import hashlib
import os
import sys

import numpy as np
import pytest

import dabtools_amd as dab
import oracle_lib as ol
from dabtools_amd import shard

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_randomised_sweep_against_the_oracle():
    """A one-minute cut of tools/stress_parity.py: captures with random ensembles (12 / 4 sub-channels), seeds, CIF counters, start
    offsets, amplitudes, noise (clean ... 9 dB), carrier offsets up to +-400 Hz and ragged lengths, decoded by the batch engine in
    parity mode; ETI bytes AND the per-call front-end trace of every capture equal or_replay's.  >= 3000 ETI frames."""
    tools = os.path.join(ROOT, "tools")                     # the sweep's oracle workers are spawned processes: they import the module by name
    sys.path.insert(0, tools)
    os.environ["PYTHONPATH"] = tools + os.pathsep + os.environ.get("PYTHONPATH", "")
    import stress_parity as sp
    from conftest import fresh_seed
    seed = fresh_seed("test_randomised_sweep_against_the_oracle")      # a fresh sweep every run; printed and kept in gpurun_out/test_seeds.txt (DABHIP_TEST_SEED replays)
    res = sp.run(rounds=2, streams=48, tfs=32, workers=min(32, os.cpu_count() or 1), seed=seed)   # (28 TF: 2956 frames in one unlucky draw of noisy captures)
    assert res["differences"] == [], (seed, res["differences"][:5])
    assert res["eti_frames_compared"] >= 3000 and res["calls_compared"] >= 2500, res
    cases = res["cases"]
    assert any(c["snr_db"] < 10 for c in cases) and any(c["bytes_cut"] for c in cases) and any(c["cfo_hz"] for c in cases)
    assert any(c["skip_samples"] for c in cases) and {c["preset"] for c in cases} == {0, 1}


def test_config2_the_benchmark_workload_itself():
    """BASELINE configs[2] as bench.py builds it: 256 distinct ensembles (seed = 2000 + stream, CIF counter 97 * stream mod 5000),
    modulated on the device, 64 TF each, resident in HBM.  (a) 16 streams spread over the batch are byte-equal to the CPU oracle's
    replay of the very bytes the device modulator wrote; (b) all 256 streams' frames are identical between the fused OFDM stage
    (default) and the two-kernel stage; (c) every stream yields 4 * (64 - 15) frames."""
    nstreams, ntf = 256, 64
    cfgs = [dab.synth_preset(0, seed=shard.stream_seed(2, g), cif_count0=(97 * g) % 5000) for g in range(nstreams)]
    nbytes = dab.synth_bytes(cfgs[0], ntf)
    bufs = [dab.DeviceBuffer(nbytes) for _ in range(nstreams)]
    dab.synth_generate_device(cfgs, ntf, [b.ptr for b in bufs], 0)
    eng = dab.Engine(0)
    ptrs, sizes = [b.ptr for b in bufs], [nbytes] * nstreams
    assert eng.decode_device(ptrs, sizes) == nstreams * 4 * (ntf - 15)
    assert eng.decoder_forms() == ({"lane"}, {"lane"})                     # the default rule at 256 streams (engine.hpp)
    digests = []
    sample = list(range(0, nstreams, 17))[:15] + [255]                     # 16 streams
    kept = {}
    for b in range(nstreams):
        eti = eng.eti(b)
        assert eti.shape == (4 * (ntf - 15), dab.ETI_BYTES), b                # (c)
        digests.append(hashlib.sha256(eti.tobytes()).digest())
        if b in sample:
            kept[b] = eti
    assert len(set(digests)) == nstreams                                     # the ensembles really are distinct
    for b in sample:                                                         # (a)
        want, _ = ol.or_replay(bufs[b].download())
        assert np.array_equal(kept[b], want), b
    eng.set_fused(False)                                                     # (b)
    assert eng.decode_device(ptrs, sizes) == nstreams * 4 * (ntf - 15)
    for b in range(nstreams):
        assert hashlib.sha256(eng.eti(b).tobytes()).digest() == digests[b], b
    eng.close()
    for b in bufs:
        b.free()


def test_bench_dump_outputs_are_the_timed_paths_frames(tmp_path):
    """`bench.py --dump-outputs DIR` at a reduced size, twice: a plain line (exactly --steps timed steps, ms_per_step, none of --full's objects),
    the same files from both runs, and their contents are the frames an engine returns for the same seeded streams."""
    import json
    import subprocess
    nstreams, ntf = 8, 20
    dumps = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--streams", str(nstreams), "--tfs", str(ntf), "--steps", "3",
                            "--warmup", "1", "--dump-outputs", str(tmp_path / run)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["config"]["eti_frames_per_step"] == nstreams * 4 * (ntf - 15)
        assert not {"roofline", "cpu_baseline", "h2d_inclusive", "two_kernel_ofdm_variant", "profile_meta"} & set(d)
        dumps.append({f: np.load(tmp_path / run / f) for f in os.listdir(tmp_path / run)})
    assert dumps[0].keys() == dumps[1].keys() and all(np.array_equal(dumps[0][f], dumps[1][f]) for f in dumps[0])
    cfgs = [dab.synth_preset(0, seed=shard.stream_seed(2, g), cif_count0=(97 * g) % 5000) for g in range(nstreams)]
    bufs = [dab.DeviceBuffer(dab.synth_bytes(c, ntf)) for c in cfgs]
    dab.synth_generate_device(cfgs, ntf, [b.ptr for b in bufs], 0)
    eng = dab.Engine(0)
    eng.decode_device([b.ptr for b in bufs], [dab.synth_bytes(c, ntf) for c in cfgs])
    eti = [eng.eti(b) for b in range(nstreams)]
    eng.close()
    for b in bufs:
        b.free()
    got = dumps[0]
    assert got["eti_frame_count.npy"].tolist() == [len(e) for e in eti]
    assert np.array_equal(got["eti_frame_digest.npy"][:, 0], np.concatenate(eti).sum(axis=1))
    idx = got["eti_frames_sample_index.npy"].astype(np.int64)
    assert len(idx) == nstreams * 4 * (ntf - 15)                              # a small output is dumped whole
    for (s, i), row in zip(idx, got["eti_frames_sample.npy"]):
        assert np.array_equal(row, eti[s][i]), (s, i)


def test_parity_guard_list_overflow_degrades_to_a_full_fp64_decision():
    """More decisions inside the fp32 error band than the guard's list holds: the launch does not fail (it did before round 3), its frames
    are decided again in full from fp64 transforms -- same ETI bytes as the oracle, fused and two-kernel OFDM stages, and a streaming
    session; guard_overflows() says how often it happened."""
    caps = [dab.synth_generate(dab.synth_preset(1, seed=1700 + i, snr_db=snr, skip_samples=sk), 24) for i, (snr, sk) in enumerate(((5.5, 0), (7.0, 31000), (1000.0, 0)))]
    wants = [ol.or_replay(c)[0] for c in caps]
    assert all(len(w) >= 24 for w in wants[1:])
    eng = dab.Engine(0)
    eng.decode(caps)
    assert eng.guard_overflows() == 0 and eng.guard_stats()[0] > 8
    eng.set_guard_list_cap(4)                                # four entries per launch: every launch with noise in it overflows
    for fused in (True, False):
        eng.set_fused(fused)
        assert eng.decode(caps) == sum(len(w) for w in wants)
        assert eng.guard_overflows() >= 1, fused              # at least the launch over the 72 MSC symbols; the FIC launch may list fewer than five
        for b, w in enumerate(wants):
            assert np.array_equal(eng.eti(b), w), (fused, b)
    eng.set_guard_list_cap(0)
    eng.set_fused(True)
    eng.decode(caps)
    assert eng.guard_overflows() == 0
    eng.close()


def test_sync_verification_fp32_first_pass_and_its_fp64_fallback():
    """K1's verification runs the coarse frequency search in single precision first and leaves a call to the fp64 pass when its arg-max is
    not clear-cut (rare: none on the benchmark workload, one of the ~120 calls of the off-tune / noisy captures below).  Three ways, one result: the default, fp64 only
    (DABHIP_VERIFY_FP32=0, the round-2 behaviour) and the test mode that hands EVERY call on to the fp64 pass (=2) -- ETI bytes and the
    per-call traces (coarse_freq_shift, fine_freq_shift ...) equal the oracle's, on off-tune captures that walk through k = +-1, 2, -6, 14."""
    import subprocess
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import dabtools_amd as dab, oracle_lib as ol
caps = [dab.synth_generate(dab.synth_preset(1, seed=1900 + i, cfo_hz=cfo, snr_db=snr, skip_samples=sk), 22)
        for i, (cfo, snr, sk) in enumerate(((1000.0, 25.0, 0), (2300.0, 25.0, 40000), (-6000.0, 20.0, 0), (13700.0, 25.0, 0), (0.0, 6.0, 0), (150.0, 1000.0, 99)))]
eng = dab.Engine(0)
eng.decode(caps)
fp64_calls = eng.stage_ms()["sync_fp64_calls"]
seen = set()
for b, iq in enumerate(caps):
    want, trace = ol.or_replay(iq)
    assert np.array_equal(eng.eti(b), want), b
    ints, ffs = eng.trace(b, len(trace))
    for k, t in enumerate(trace):
        assert tuple(ints[k]) == (t.ok, t.read_frame, t.coarse_timeshift, t.fine_timeshift, t.coarse_freq_shift, t.fifo_count), (b, k)
        assert abs(ffs[k] - t.fine_freq_shift) < 1e-9, (b, k)
        seen.add(t.coarse_freq_shift)
assert {1, 2, -6, 14} <= seen, seen
print("ok fp64_calls=%%d" %% fp64_calls)
""" % (ROOT, os.path.join(ROOT, "tests"))
    out = {}
    for mode in ("1", "0", "2"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DABHIP_VERIFY_FP32=mode), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0 and "ok fp64_calls=" in r.stdout, (mode, r.stdout[-500:], r.stderr[-2000:])
        out[mode] = int(r.stdout.strip().rsplit("=", 1)[1])
    assert out["1"] <= 5 and out["0"] == 0 and out["2"] > 50, out      # default: at most a handful of the ~120 calls are not clear-cut (off-tune by 14 carriers, 6 dB)


def test_exact_zero_products_are_decided_as_the_reference_decides_them():
    """Two whole OFDM symbols of a locked capture replaced by the byte 127 (sample value 0): the transform of the second one is exactly
    zero, so every differential product of that symbol and of the next is an exact +-0 -- where the sign bit of the product (what the
    guarded fused kernel writes, round 3) and the reference's comparisons `re > 0`, `im > 0` (input_sdr.c:157-158) part ways.  Such
    decisions are always listed for the fp64 re-decision (also when the symbol's error bound is zero): ETI byte-equal to the oracle, with
    the fused kernel and with the two-kernel stage."""
    cfg = dab.synth_preset(1, seed=8801, cif_count0=40, snr_db=1000.0)
    iq = dab.synth_generate(cfg, 24).copy()
    for tf, sym in ((15, 40), (18, 4), (20, 74)):          # an MSC symbol pair in mid-frame, the first MSC symbols, the last two of a frame
        a = 2 * (tf * 196608 + 2656 + sym * 2552)
        iq[a: a + 2 * 2 * 2552] = 127
    want, _ = ol.or_replay(iq)
    assert len(want) >= 4 * (24 - 16)
    eng = dab.Engine(0)
    for fused in (True, False):
        eng.set_fused(fused)
        assert eng.decode([iq]) == len(want)
        assert np.array_equal(eng.eti(0), want), fused
        if fused:
            assert eng.guard_stats()[0] >= 3 * 1536            # at least the carriers of three all-zero symbols were listed and re-decided
    eng.close()
