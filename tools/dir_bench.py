#!/usr/bin/env python3
"""Time the ensemble directory stage (dabtools_amd.Dir) at full batch: B streams x F ETI frames whose FIC bytes are the modulator's si_mode
carousel of preset 0 (every frame of the rest is zero: the stage reads bytes 5, 6 and the FIC only), frames in device memory.

  python tools/dir_bench.py [--streams 256] [--frames 256] [--reps 7]

Prints one JSON line: wall time of a push (min / median / max over the reps after one warm-up push), the GPU time per stage of the median
push, the facts per push and whether every stream's directory is complete."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dabtools_amd as dab  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    cfg = dab.synth_preset(0, seed=1)
    cfg.dabplus_slots, cfg.packet_slots, cfg.packet_fec_slots, cfg.ts_slots = 1 << 1, 1 << 2 | 1 << 4, 1 << 2, 1 << 3
    cfg.si_mode = 1
    one = np.zeros((a.frames, dab.ETI_BYTES), dtype=np.uint8)
    nst = cfg.nsub
    one[:, 5] = 0x80 | nst
    one[:, 6] = 1 << 3
    for f in range(a.frames):
        one[f, 12 + 4 * nst:12 + 4 * nst + 96] = dab.synth_fibs(cfg, f)
    flat = np.tile(one.reshape(-1), a.streams)
    buf = dab.DeviceBuffer(flat.size)
    buf.upload(flat)
    d = dab.Dir(a.streams)
    counts = [a.frames] * a.streams
    d.push((buf.ptr, counts))
    walls, stages = [], []
    for _ in range(a.reps):
        t = time.perf_counter()
        d.push((buf.ptr, counts))
        walls.append((time.perf_counter() - t) * 1e3)
        stages.append(d.stage_ms())
    order = np.argsort(walls)
    st = d.stats(a.streams - 1)
    print(json.dumps({"streams": a.streams, "frames": a.frames, "push_ms": {"min": round(min(walls), 3), "median": round(float(np.median(walls)), 3), "max": round(max(walls), 3)},
                      "stage_ms": {k: round(v, 3) for k, v in stages[order[len(order) // 2]].items()},
                      "facts_per_push": int(st[8]) // (a.reps + 1) * a.streams, "complete": all(d.complete(b) for b in (0, a.streams - 1))}))
    d.close()
    buf.free()


if __name__ == "__main__":
    main()
