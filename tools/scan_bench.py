"""Cost of the block scan (dabhip_scan_push) at full batch: 256 streams x 64 segments of 4096 samples resident in device memory, cs16 and cu8.
Prints one JSON object: ms per push (wall clock around the synchronous call, and the stage's own GPU times), bytes in / transform time beside the
bare copy rate of the same run (dabhip_stream_ceiling, k_probe.hip), and the butterflies per second.

  python tools/scan_bench.py [--streams 256] [--segments 64] [--reps 5] [--out FILE]

The inputs are random samples; the stage's time does not depend on their values.  A fresh object per repetition: every push is a stream's first and
fills its window.  Under `rocprofv3 --kernel-trace --stats` the run gives the per-kernel times."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dabtools_amd as dab  # noqa: E402

CASES = (("cs16", 10000000), ("cu8", 10000000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available() or dab.lib().dabhip_device_count() <= 0:
        raise SystemExit("scan_bench: no GPU (there is nothing to measure without one)")
    dev = torch.device("cuda", 0)
    result = {"streams": a.streams, "segments_per_stream": a.segments, "reps": a.reps, "device": dab.device_identity(0)[1]}
    result["stream_ceiling_gbs"] = dab.stream_ceiling(0, 4 << 30, 3)
    result["cases"] = []
    nsamples = a.segments * dab.SCAN_BINS
    for fmt, rate in CASES:
        data = torch.empty((a.streams, 2 * nsamples), dtype=torch.uint8 if fmt == "cu8" else torch.int16, device=dev)
        if fmt == "cu8":
            data.random_(0, 256)
        else:
            data.random_(-8000, 8000)
        row_bytes = data.element_size() * 2 * nsamples
        ptrs = [data.data_ptr() + b * row_bytes for b in range(a.streams)]
        sizes = [row_bytes] * a.streams
        torch.cuda.synchronize(dev)
        walls, stages = [], []
        for r in range(a.reps + 1):
            scan = dab.Scan(0, a.streams, fmt, rate, a.segments)
            t0 = time.perf_counter()
            done = scan.push_ptrs(ptrs, sizes, on_device=True)
            wall = (time.perf_counter() - t0) * 1e3
            assert done == a.streams * a.segments
            if r:                                     # the first one loads the code object
                walls.append(wall)
                stages.append(scan.stage_ms())
            scan.close()
        k = walls.index(min(walls))
        transform_ms = min(s["transform"] for s in stages)
        bytes_in = a.streams * row_bytes
        butterflies = a.streams * a.segments * 12 * 2048
        result["cases"].append({
            "format": fmt, "rate_hz": rate, "input_samples_per_stream": nsamples, "bytes_in": bytes_in,
            "push_ms_best": walls[k], "push_ms_median": sorted(walls)[len(walls) // 2], "stage_ms_of_best": stages[k],
            "transform_kernel_ms_best": transform_ms,
            "gbs_transform_kernel": bytes_in / (transform_ms * 1e-3) / 1e9,
            "transform_kernel_vs_copy_rate": bytes_in / (transform_ms * 1e-3) / 1e9 / result["stream_ceiling_gbs"]["copy"],
            "butterflies": butterflies, "gbutterflies_per_s_transform_kernel": butterflies / (transform_ms * 1e-3) / 1e9,
            "msamples_per_s_transform_kernel": a.streams * nsamples / (transform_ms * 1e-3) / 1e6,
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
