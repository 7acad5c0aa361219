"""Cost of the ingest stage (dabhip_ingest_push) at full batch: 256 streams x 64 TF worth of input resident in device memory, for cu8 and cs16 at
2.4 Msps and cs16 at 10 Msps.  Prints one JSON object: ms per push (wall clock around the synchronous call, and the stage's own GPU times),
(bytes in + bytes out) / time beside the bare copy rate of the same run (dabhip_stream_ceiling, k_probe.hip), and the ratio to the decode step of
the same batch (256 synthetic preset-0 ensembles x 64 TF, Engine.decode_device, timed in this run).

  python tools/ingest_bench.py [--streams 256] [--tf 64] [--reps 5] [--out FILE]

The inputs are random samples (every stream its own buffer: 15 GB of cs16 at 2.4 Msps do not fit any cache); the stage's time does not depend on
their values.  Explicit gain, so that the energy reduction (once per stream's life) is not in the figure; one untimed push with automatic gain is
reported beside it.  Under `rocprofv3 --kernel-trace --stats` the run gives the per-kernel times."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dabtools_amd as dab  # noqa: E402
from dabtools_amd import shard  # noqa: E402

TF_SAMPLES = 196608
CASES = (("cu8", 2400000), ("cs16", 2400000), ("cs16", 10000000))


def decode_step_ms(torch, dev, nstreams, ntf, reps):
    cfgs = [dab.synth_preset(0, seed=shard.stream_seed(2, g), cif_count0=(97 * g) % 5000) for g in range(nstreams)]
    tensors = [torch.empty(dab.synth_bytes(c, ntf), dtype=torch.uint8, device=dev) for c in cfgs]
    dab.synth_generate_device(cfgs, ntf, [t.data_ptr() for t in tensors], 0)
    eng = dab.Engine(0)
    args = dab.Engine.marshal([t.data_ptr() for t in tensors], [t.numel() for t in tensors])
    frames = eng.decode_marshalled(args)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        eng.decode_marshalled(args)
        times.append((time.perf_counter() - t0) * 1e3)
    eng.close()
    del tensors
    torch.cuda.empty_cache()
    return min(times), sorted(times)[len(times) // 2], frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--tf", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available() or dab.lib().dabhip_device_count() <= 0:
        raise SystemExit("ingest_bench: no GPU (there is nothing to measure without one)")
    dev = torch.device("cuda", 0)
    result = {"streams": a.streams, "tf_per_stream": a.tf, "reps": a.reps, "device": dab.device_identity(0)[1]}
    result["stream_ceiling_gbs"] = dab.stream_ceiling(0, 4 << 30, 3)
    best, median, frames = decode_step_ms(torch, dev, a.streams, a.tf, a.reps)
    result["decode_step"] = {"ms_best": best, "ms_median": median, "eti_frames": frames,
                             "what": "Engine.decode_device of %d preset-0 ensembles x %d TF resident in HBM, wall clock" % (a.streams, a.tf)}
    result["cases"] = []
    for fmt, rate in CASES:
        _, L, M, T = dab.ingest_taps(fmt, rate)
        nsamples = a.tf * TF_SAMPLES * M // L
        data = torch.empty((a.streams, 2 * nsamples), dtype=torch.uint8 if fmt == "cu8" else torch.int16, device=dev)
        for b in range(0, a.streams, 16):             # in slices: the generator's temporaries stay small
            if fmt == "cu8":
                data[b:b + 16].random_(0, 256)
            else:
                data[b:b + 16].random_(-8000, 8000)
        row_bytes = data.element_size() * 2 * nsamples
        ptrs = [data.data_ptr() + b * row_bytes for b in range(a.streams)]
        sizes = [row_bytes] * a.streams
        torch.cuda.synchronize(dev)
        walls, stages, out_bytes = [], [], 0
        for r in range(a.reps + 1):                   # a fresh object per repetition: every push is a stream's first, the same work each time
            ing = dab.Ingest(0, a.streams, fmt, rate, 256)
            t0 = time.perf_counter()
            out_bytes = ing.push_ptrs(ptrs, sizes, on_device=True)
            wall = (time.perf_counter() - t0) * 1e3
            if r:                                     # the first one allocates the output and loads the code object
                walls.append(wall)
                stages.append(ing.stage_ms())
            ing.close()
        ing = dab.Ingest(0, a.streams, fmt, rate, 0)
        t0 = time.perf_counter()
        ing.push_ptrs(ptrs, sizes, on_device=True)
        auto_wall = (time.perf_counter() - t0) * 1e3
        auto_stage = ing.stage_ms()
        ing.close()
        k = walls.index(min(walls))
        moved = a.streams * row_bytes + out_bytes
        resample_ms = min(s["resample"] for s in stages)
        result["cases"].append({
            "format": fmt, "rate_hz": rate, "L": L, "M": M, "taps_per_phase": T, "input_samples_per_stream": nsamples,
            "bytes_in": a.streams * row_bytes, "bytes_out": out_bytes,
            "push_ms_best": walls[k], "push_ms_median": sorted(walls)[len(walls) // 2], "stage_ms_of_best": stages[k],
            "resample_kernel_ms_best": resample_ms,
            "gbs_push": moved / (walls[k] * 1e-3) / 1e9, "gbs_resample_kernel": moved / (resample_ms * 1e-3) / 1e9,
            "resample_kernel_vs_copy_rate": moved / (resample_ms * 1e-3) / 1e9 / result["stream_ceiling_gbs"]["copy"],
            "multiply_accumulates": out_bytes * T, "gmacs_per_s_resample_kernel": out_bytes * T / (resample_ms * 1e-3) / 1e9,
            "push_vs_decode_step": walls[k] / best,
            "first_push_with_automatic_gain": {"push_ms": auto_wall, "stage_ms": auto_stage},
        })
        del data
        torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
