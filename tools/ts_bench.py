"""Cost of the MPEG-2 TS stage (dabhip_ts_push) at full batch, beside the decode step of the same run: 256 streams x 64 TF (256 ETI frames
each) of the preset-0 ensemble with every slot a TS slot, resident in device memory as Engine.eti_device_ptr leaves them.

  python tools/ts_bench.py [--rounds 3] [--streams 256] [--tf 64] [--reps 10] [--byte-error-rate 5e-3] [--parent-tree DIR] [--out FILE]

Every measurement is a process of its own, and the kinds alternate round by round: the stage clean, the stage with random byte errors in the
sub-channel bytes, the decode step of this build (bench.py, the stage unused) and, with --parent-tree, the decode step of another built checkout
(the parent commit's) through that checkout's own bench.py and binding.  Prints one JSON object with every round's figures, their medians and spreads, the
per-stage GPU times from dabhip_ts_stage_ms (one stage per kernel; locate includes the layout pass, jobs the scan), and the ratio to the decode step.

The frames are built on the host from the synthetic modulator's payloads (one ensemble, its 256 frames repeated for every stream), so the stage's
processes need no IQ and no decode."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def child_stage(a, rate):
    import dabplus_model as dm
    import dabtools_amd as dab
    nf = 4 * a.tf
    cfg = dab.synth_preset(0, seed=1)
    cfg.ts_slots = (1 << cfg.nsub) - 1
    cfg.ts_phase = 17
    ids = [cfg.sub[k].id for k in range(cfg.nsub)]
    one = np.stack([dm.eti_frame(c % 250, [(ids[k], dab.synth_payload(cfg, c, k)) for k in range(cfg.nsub)]) for c in range(nf)])
    pay0 = 12 + 4 * len(ids) + 96
    pay_bytes = sum(dab.synth_payload(cfg, 0, k).size for k in range(cfg.nsub))
    frames = np.tile(one, (a.streams, 1))
    if rate > 0:
        rng = np.random.default_rng(3)
        region = frames[:, pay0:pay0 + pay_bytes]
        hit = rng.random(region.shape) < rate
        region[hit] ^= rng.integers(1, 256, int(hit.sum())).astype(np.uint8)
        frames[:, pay0:pay0 + pay_bytes] = region
    buf = dab.DeviceBuffer(frames.size)
    buf.upload(frames)
    counts = [nf] * a.streams
    walls, stages = [], []
    # a fresh handle per repetition.  The timed push continues the stream with the same 256 frames again, so at the seam every lane sees words
    # that fail, two missed slots and a sync loss, and searches its run flags again, clean run included: the counters show them
    for r in range(a.reps + 1):
        pk = dab.Ts(a.streams, ids)
        pk.push((buf.ptr, counts))                                     # the first push allocates; the timed one goes on with the same frames again
        t = time.perf_counter()
        npk = pk.push((buf.ptr, counts))
        w = (time.perf_counter() - t) * 1e3
        if r:
            walls.append(w)
            stages.append(pk.stage_ms())
        if r == a.reps:
            stats = np.sum([pk.stats(b, q) for b in range(0, a.streams, max(1, a.streams // 8)) for q in range(len(ids))], axis=0)
        pk.close()
    st = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
    print(json.dumps({"push_ms_median": float(np.median(walls)), "push_ms_min": float(np.min(walls)), "gpu_ms_median": float(sum(st.values())),
                      "stage_ms_median": st, "packets_per_push": int(npk), "subchannel_bytes": a.streams * nf * pay_bytes,
                      "counters_of_every_8th_stream": dict(zip(dab.TS_STATS, [int(x) for x in stats]))}))


def run_child(args, env=None):
    out = subprocess.run([sys.executable] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=900)
    if out.returncode != 0:
        raise SystemExit("child failed: %s\n%s" % (" ".join(args), out.stderr[-2000:]))
    return json.loads([line for line in out.stdout.splitlines() if line.startswith("{")][-1])


def spread(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values)), "rounds": [float(v) for v in values]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--tf", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--byte-error-rate", type=float, default=5e-3)
    ap.add_argument("--bench-steps", type=int, default=10)
    ap.add_argument("--bench-warmup", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child is not None:
        return child_stage(a, float(a.child))
    me = [os.path.abspath(__file__), "--streams", str(a.streams), "--tf", str(a.tf), "--reps", str(a.reps)]
    bench = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup), "--no-cpu-baseline", "--no-variants"]
    rounds = {"clean": [], "byte_errors": [], "decode": [], "decode_parent": []}

    def measure(kind, args):
        rounds[kind].append(run_child(args))
        print("round %d: %s done" % (len(rounds[kind]), kind), file=sys.stderr, flush=True)

    for _ in range(a.rounds):
        measure("clean", me + ["--child", "0"])
        measure("decode", bench)
        measure("byte_errors", me + ["--child", str(a.byte_error_rate)])
        if a.parent_tree:
            measure("decode_parent", [os.path.join(os.path.abspath(a.parent_tree), "bench.py")] + bench[1:])
    result = {"streams": a.streams, "tf_per_stream": a.tf, "rounds": a.rounds, "byte_error_rate": a.byte_error_rate,
              "decode_step_ms": spread([r["ms_per_step"] for r in rounds["decode"]]),
              "decode_step_ms_is": "bench.py --gpus 1 ms_per_step of this build in the same rounds, the TS stage unused"}
    if a.parent_tree:
        result["decode_step_ms_parent_build"] = spread([r["ms_per_step"] for r in rounds["decode_parent"]])
    step = result["decode_step_ms"]["median"]
    for name in ("clean", "byte_errors"):
        last = rounds[name][-1]
        result[name] = {"push_ms": spread([r["push_ms_median"] for r in rounds[name]]), "gpu_ms": spread([r["gpu_ms_median"] for r in rounds[name]]),
                        "stage_ms_median_of_rounds": {k: float(np.median([r["stage_ms_median"][k] for r in rounds[name]])) for k in last["stage_ms_median"]},
                        "packets_per_push": last["packets_per_push"], "subchannel_bytes": last["subchannel_bytes"],
                        "counters_of_every_8th_stream": last["counters_of_every_8th_stream"]}
        result[name]["push_over_decode_step"] = result[name]["push_ms"]["median"] / step
    result["packet_stage_push_over_decode_step"] = {"clean": 0.43, "byte_errors": 0.59, "from": "profiles/r16_packet_stage.json"}
    print(json.dumps(result, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
