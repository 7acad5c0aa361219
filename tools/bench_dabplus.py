"""Cost of the DAB+ stage (dabhip_dabplus_push) at full batch: 256 streams x 64 TF (256 ETI frames each) of the preset-0 ensemble with every slot
DAB+, resident in device memory as Engine.eti_device_ptr leaves them.  Prints one JSON object: push wall time and per-stage GPU time, clean and with
random byte errors in the sub-channel bytes, against the decode step of profiles/r06_bench.json.

  python tools/bench_dabplus.py [--streams 256] [--tf 64] [--reps 10] [--byte-error-rate 5e-3] [--out FILE]

The frames are built on the host from the synthetic modulator's protected payloads (one ensemble, its 256 frames repeated for every stream), so the
run needs no IQ and no decode; under `rocprofv3 --kernel-trace --stats` it gives the per-kernel times."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dabplus_model as m  # noqa: E402
import dabtools_amd as dab  # noqa: E402


def ensemble_frames(nframes, seed=1):
    cfg = dab.synth_preset(0, seed=seed)
    cfg.dabplus_slots = (1 << cfg.nsub) - 1
    ids = [cfg.sub[k].id for k in range(cfg.nsub)]
    frames = np.stack([m.eti_frame(c % 250, [(ids[k], dab.synth_payload(cfg, c, k)) for k in range(cfg.nsub)]) for c in range(nframes)])
    return frames, ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--tf", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--byte-error-rate", type=float, default=5e-3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nf = 4 * a.tf
    one, ids = ensemble_frames(nf)
    pay0 = 12 + 4 * len(ids) + 96
    pay_bytes = int(sum((int(f[8 + 4 * i + 2]) & 3) << 8 | int(f[8 + 4 * i + 3]) for i, f in [(i, one[0]) for i in range(len(ids))])) * 8
    result = {"streams": a.streams, "tf_per_stream": a.tf, "eti_frames": a.streams * nf, "subchannels_per_stream": len(ids),
              "subchannel_bytes": a.streams * nf * pay_bytes, "syndrome_macs": a.streams * nf * pay_bytes * 10}
    rng = np.random.default_rng(3)
    for name, rate in (("clean", 0.0), ("byte_errors", a.byte_error_rate)):
        frames = np.tile(one, (a.streams, 1))
        if rate > 0:
            region = frames[:, pay0:pay0 + pay_bytes]
            hit = rng.random(region.shape) < rate
            region[hit] ^= rng.integers(1, 256, int(hit.sum())).astype(np.uint8)
            frames[:, pay0:pay0 + pay_bytes] = region
        buf = dab.DeviceBuffer(frames.size)
        buf.upload(frames)
        dp = dab.DabPlus(a.streams, ids)
        counts = [nf] * a.streams
        walls, stages = [], []
        for r in range(a.reps + 1):
            t = time.perf_counter()
            nsf = dp.push((buf.ptr, counts))
            w = (time.perf_counter() - t) * 1e3
            if r:                                                          # the first push allocates the buffers
                walls.append(w)
                stages.append(dp.stage_ms())
        st = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
        stats = np.sum([dp.stats(b, q) for b in range(a.streams) for q in range(len(ids))], axis=0)
        result[name] = {"push_ms_median": float(np.median(walls)), "push_ms_min": float(np.min(walls)), "gpu_ms_median": float(sum(st.values())),
                        "stage_ms_median": st, "superframes_per_push": int(nsf),
                        "counters_all_pushes": dict(zip(dab.DABPLUS_STATS, [int(x) for x in stats]))}
        dp.close()
        buf.free()
    bench = json.load(open(os.path.join(ROOT, "profiles", "r06_bench.json")))
    result["decode_step_ms"] = bench["ms_per_step"]
    result["decode_step_ms_is"] = "profiles/r06_bench.json ms_per_step (256 streams, the default bench.py step)"
    for name in ("clean", "byte_errors"):
        result[name]["push_over_decode_step"] = result[name]["push_ms_median"] / bench["ms_per_step"]
    print(json.dumps(result, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
