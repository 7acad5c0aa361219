"""Cost of the ingest stage's tuned mode (dabhip_ingest_create_tuned) at full batch: 256 OUTPUT streams x 64 TF worth of output, the wideband input
resident in device memory, for cs16 at 10 Msps with 5 channels (52 input streams: 260 outputs, scaled to 256) and cs8 at 8 Msps with 4 channels
(64 input streams).  The yardstick is the plain ingest stage at the same format and rate in the same run, scaled to the same number of output
streams.  Prints one JSON object: ms per push (wall clock around the synchronous call, and the stage's own GPU times), both figures and their ratio.

  python tools/tune_bench.py [--outputs 256] [--tf 64] [--reps 5] [--out profiles/r13_tune_stage.json]

The inputs are random samples (every stream its own buffer); the stage's time does not depend on their values.  Explicit gain, so that the energy
pass (once per stream's life) is not in the figure; one untimed push with automatic gain is reported beside it.  Under
`rocprofv3 --kernel-trace --stats` the run gives the per-kernel times."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dabtools_amd as dab  # noqa: E402

TF_SAMPLES = 196608
# format, rate, the channels' offsets: five Band III blocks 1.712 MHz apart in 10 Msps, four in 8 Msps
CASES = (("cs16", 10000000, (-3424000, -1712000, 0, 1712000, 3424000)), ("cs8", 8000000, (-2568000, -856000, 856000, 2568000)))


def time_pushes(make, ptrs, sizes, reps):
    """A fresh object per repetition (every push is a stream's first: the same work each time); the first one allocates and loads the code object."""
    walls, stages, out_bytes = [], [], 0
    for r in range(reps + 1):
        ing = make(256)
        t0 = time.perf_counter()
        out_bytes = ing.push_ptrs(ptrs, sizes, on_device=True)
        wall = (time.perf_counter() - t0) * 1e3
        if r:
            walls.append(wall)
            stages.append(ing.stage_ms())
        ing.close()
    ing = make(0)
    t0 = time.perf_counter()
    ing.push_ptrs(ptrs, sizes, on_device=True)
    auto = {"push_ms": (time.perf_counter() - t0) * 1e3, "stage_ms": ing.stage_ms()}
    ing.close()
    k = walls.index(min(walls))
    return {"push_ms_best": walls[k], "push_ms_median": sorted(walls)[len(walls) // 2], "stage_ms_of_best": stages[k],
            "resample_kernel_ms_best": min(s["resample"] for s in stages), "bytes_out": out_bytes, "first_push_with_automatic_gain": auto}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--outputs", type=int, default=256)
    ap.add_argument("--tf", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available() or dab.lib().dabhip_device_count() <= 0:
        raise SystemExit("tune_bench: no GPU (there is nothing to measure without one)")
    dev = torch.device("cuda", 0)
    result = {"output_streams": a.outputs, "tf_per_output_stream": a.tf, "reps": a.reps, "device": dab.device_identity(0)[1], "cases": []}
    for fmt, rate, offsets in CASES:
        _, L, M, T = dab.ingest_tune_taps(fmt, rate)
        plain_T = dab.ingest_taps(fmt, rate)[3]
        nch = len(offsets)
        nin = -(-a.outputs // nch)                        # input streams of the tuned run; the plain run takes as many
        nsamples = a.tf * TF_SAMPLES * M // L
        data = torch.empty((nin, 2 * nsamples), dtype=torch.int8 if fmt == "cs8" else torch.int16, device=dev)
        for b in range(0, nin, 16):                       # in slices: the generator's temporaries stay small
            data[b:b + 16].random_(-100, 100) if fmt == "cs8" else data[b:b + 16].random_(-8000, 8000)
        row_bytes = data.element_size() * 2 * nsamples
        ptrs = [data.data_ptr() + b * row_bytes for b in range(nin)]
        sizes = [row_bytes] * nin
        torch.cuda.synchronize(dev)
        tuned = time_pushes(lambda g: dab.Ingest(0, nin, fmt, rate, g, offsets=offsets), ptrs, sizes, a.reps)
        plain = time_pushes(lambda g: dab.Ingest(0, nin, fmt, rate, g), ptrs, sizes, a.reps)
        tuned_ms = tuned["push_ms_best"] * a.outputs / (nin * nch)       # both scaled to a.outputs output streams
        plain_ms = plain["push_ms_best"] * a.outputs / nin
        result["cases"].append({
            "format": fmt, "rate_hz": rate, "offsets_hz": list(offsets), "L": L, "M": M, "taps_per_phase_tuned": T, "taps_per_phase_plain": plain_T,
            "input_streams": nin, "channels": nch, "input_samples_per_stream": nsamples, "bytes_in": nin * row_bytes,
            "tuned": tuned, "plain": plain,
            "tuned_ms_per_push_at_%d_outputs" % a.outputs: tuned_ms, "plain_ms_per_push_at_%d_outputs" % a.outputs: plain_ms,
            "tuned_over_plain_per_output_stream": tuned_ms / plain_ms,
            "multiply_accumulates_tuned": tuned["bytes_out"] * T,
            "gmacs_per_s_tuned_kernel": tuned["bytes_out"] * T / (tuned["resample_kernel_ms_best"] * 1e-3) / 1e9,
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
