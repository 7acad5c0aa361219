"""Cost of transmitter identification (dabhip_engine_set_tii) at full batch: 256 streams x 64 TF resident in device memory, the whole decode step
with TII on and with TII off, and the TII kernel's own GPU time (dabhip_engine_tii_ms), in interleaved rounds on one box.  With --parent-tree DIR
(a built checkout of the commit before TII existed) every round also runs that tree's library, so that "TII off" can be held against it: the two
medians must lie within the rounds' own spread.  Prints one JSON object.

  python tools/tii_bench.py [--streams 256] [--tfs 64] [--rounds 3] [--steps 5] [--warmup 2] [--parent-tree DIR] [--out FILE]

Every measurement is a child process of its own (one library per process), which modulates its streams on the GPU (the null symbols are silent: the
stage's time does not depend on their content), decodes --warmup + --steps times and reports the wall clock of each timed step."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker(a):
    sys.path.insert(0, a.tree)
    import dabtools_amd as dab
    from dabtools_amd import shard
    if dab.lib().dabhip_device_count() <= 0:
        raise SystemExit("tii_bench: no GPU (there is nothing to measure without one)")
    cfgs = [dab.synth_preset(0, seed=shard.stream_seed(2, g), cif_count0=(97 * g) % 5000) for g in range(a.streams)]
    bufs = [dab.DeviceBuffer(dab.synth_bytes(c, a.tfs)) for c in cfgs]
    dab.synth_generate_device(cfgs, a.tfs, [b.ptr for b in bufs], 0)
    eng = dab.Engine(0)
    if a.tii:
        eng.set_tii(True)
    ptrs, sizes = [b.ptr for b in bufs], [b.nbytes for b in bufs]
    steps, tii_ms, frames = [], [], 0
    for k in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        frames = eng.decode_device(ptrs, sizes)
        ms = (time.perf_counter() - t0) * 1e3
        if k >= a.warmup:
            steps.append(ms)
            tii_ms.append(eng.tii_ms() if a.tii else 0.0)
    out = {"step_ms": steps, "tii_ms": tii_ms, "eti_frames": int(frames), "device": dab.device_identity(0)[1]}
    if a.tii:
        out["frames_counted"] = sum(eng.tii_sums(b)[1] for b in range(a.streams))
    print("RESULT " + json.dumps(out))


def run_child(a, tree, tii):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--tii", str(int(tii)), "--streams", str(a.streams), "--tfs", str(a.tfs),
           "--steps", str(a.steps), "--warmup", str(a.warmup)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("tii_bench: a measurement failed (rc %d): %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def summary(runs):
    steps = [v for r in runs for v in r["step_ms"]]
    per_round = [statistics.median(r["step_ms"]) for r in runs]
    return {"step_ms_median": statistics.median(steps), "step_ms_min": min(steps), "step_ms_max": max(steps), "round_medians": per_round,
            "round_spread_ms": max(per_round) - min(per_round), "eti_frames": runs[0]["eti_frames"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--tfs", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--tii", type=int, default=0)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    variants = [("tii_off", ROOT, False), ("tii_on", ROOT, True)] + ([("parent", a.parent_tree, False)] if a.parent_tree else [])
    runs = {name: [] for name, _, _ in variants}
    for r in range(a.rounds):
        for name, tree, tii in (variants if r % 2 == 0 else variants[::-1]):      # interleaved, and the order turned round every other round
            runs[name].append(run_child(a, tree, tii))
    result = {"streams": a.streams, "tfs_per_stream": a.tfs, "rounds": a.rounds, "steps_per_round": a.steps, "warmup": a.warmup, "device": runs["tii_off"][0]["device"]}
    for name in runs:
        result[name] = summary(runs[name])
    on = runs["tii_on"]
    kernel = [v for r in on for v in r["tii_ms"]]
    result["tii_on"]["tii_kernel_ms_median"] = statistics.median(kernel)
    result["tii_on"]["tii_kernel_ms_min"] = min(kernel)
    result["tii_on"]["frames_counted"] = on[0]["frames_counted"]
    result["tii_on_minus_off_ms"] = result["tii_on"]["step_ms_median"] - result["tii_off"]["step_ms_median"]
    if a.parent_tree:
        spread = max(result["tii_off"]["round_spread_ms"], result["parent"]["round_spread_ms"])
        diff = result["tii_off"]["step_ms_median"] - result["parent"]["step_ms_median"]
        result["off_minus_parent_ms"] = diff
        result["off_within_spread_of_parent"] = abs(diff) <= spread
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
