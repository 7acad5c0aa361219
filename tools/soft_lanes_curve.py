#!/usr/bin/env python3
"""tools/soft_lanes_curve.py -- what the soft four-lane decoder (vit_soft_lanes.hpp) gains over the soft lane form, by batch size.

B in {8, 16, 32, 64} streams x --tfs TF of the benchmark ensemble at --snr dB (IQ resident in HBM, device modulator), a soft engine with
set_soft_lanes(True), every batch decoded in three configurations: (MSC, FIC) = (lane, lane) -- the baseline, the same build's lane form on
the same box --, (four, lane) and (lane, four).  The configurations take turns, --rounds rounds of --steps decodes each on ONE box in ONE
process, so that drift hits them alike; per configuration and round: ms per decode (wall clock around the steps) and the engine's stage
times.  The MSC knob is judged on the "viterbi" stage and the whole decode of (four, lane) against (lane, lane), the FIC knob on the "fic"
stage and the whole decode of (lane, four).  "wins" = the median over the rounds is lower than the baseline's by more than the spread (max -
min over the rounds) of either configuration, for the stage AND the whole decode.  One JSON document on stdout
(profiles/r08_soft_lanes_curve.json); the defaults of DABHIP_VIT_SOFT_FOUR_LANES / DABHIP_FIC_SOFT_FOUR_LANES in decoder_form.hpp are the
group / tile counts of the largest batch that wins, or 0."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = (("lane", "lane"), ("four", "lane"), ("lane", "four"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tfs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--snr", type=float, default=5.0)
    ap.add_argument("--batches", type=str, default="8,16,32,64")
    args = ap.parse_args()
    import torch
    import dabtools_amd as dab
    from dabtools_amd import payload

    batches = [int(x) for x in args.batches.split(",")]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cfgs = [payload.bench_cfg(dab, i, args.snr) for i in range(max(batches))]
    tensors = [torch.empty(dab.synth_bytes(c, args.tfs), dtype=torch.uint8, device=dev) for c in cfgs]
    dab.synth_generate_device(cfgs, args.tfs, [t.data_ptr() for t in tensors], 0)
    torch.cuda.synchronize()
    ptrs, sizes = [t.data_ptr() for t in tensors], [t.numel() for t in tensors]
    eng = dab.Engine(0)
    eng.set_soft(True)
    eng.set_soft_lanes(True)
    rows = []
    for B in batches:
        call = eng.marshal(ptrs[:B], sizes[:B])
        per = {c: {"ms_per_decode": [], "viterbi_ms": [], "fic_ms": []} for c in CONFIGS}
        frames_of, ran = {}, {}
        for c in CONFIGS:                                      # warm-up, and what ran
            eng.set_decoder_forms(*c)
            for _ in range(2):
                frames_of[c] = eng.decode_marshalled(call)
            ran[c] = [sorted(s) for s in eng.decoder_forms()]
        # what the rule in decoder_form.hpp is given for this batch: the MSC batch's groups of 64 code words (msc_plan), and the FIC's tiles of 64
        # blocks (one fic_group launch per tile with the launch limit at 1; the output does not depend on the limit)
        msc_groups = len(eng.msc_plan()[0])
        eng.set_launch_limits(fic_group_tiles=1)
        eng.decode_marshalled(call)
        fic_tiles = eng.launch_report()["fic_group"]
        eng.set_launch_limits()
        for _ in range(args.rounds):
            for c in CONFIGS:
                eng.set_decoder_forms(*c)
                eng.decode_marshalled(call)
                torch.cuda.synchronize()
                stage = {}
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    eng.decode_marshalled(call)
                    for k, v in eng.stage_ms().items():
                        stage[k] = stage.get(k, 0.0) + v
                torch.cuda.synchronize()
                per[c]["ms_per_decode"].append(1e3 * (time.perf_counter() - t0) / args.steps)
                per[c]["viterbi_ms"].append(stage.get("viterbi", 0.0) / args.steps)
                per[c]["fic_ms"].append(stage.get("fic", 0.0) / args.steps)
        report = eng.launch_report()

        def summary(c):
            return {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in per[c].items()}

        def wins(c, stage_key):
            base = per[CONFIGS[0]]
            ok = True
            for key in (stage_key, "ms_per_decode"):
                spread = max(max(base[key]) - min(base[key]), max(per[c][key]) - min(per[c][key]))
                ok = ok and statistics.median(base[key]) - statistics.median(per[c][key]) > spread
            return ok

        row = {"streams": B, "tf_per_stream": args.tfs, "eti_frames_per_decode": frames_of[CONFIGS[0]],
               "same_frame_count_in_every_configuration": len(set(frames_of.values())) == 1,
               "forms_ran": {"/".join(c): ran[c] for c in CONFIGS},
               "msc_groups": msc_groups, "fic_tiles": fic_tiles,
               "lane_lane": summary(CONFIGS[0]), "four_lane": summary(CONFIGS[1]), "lane_four": summary(CONFIGS[2]),
               "msc_four_wins": wins(CONFIGS[1], "viterbi_ms"), "fic_four_wins": wins(CONFIGS[2], "fic_ms")}
        row["launch_report_last"] = {k: v for k, v in report.items() if v}
        rows.append(row)
        print("B=%3d  viterbi lane %.3f four %.3f ms | fic lane %.3f four %.3f ms | decode lane/lane %.3f four/lane %.3f lane/four %.3f ms  msc wins %s fic wins %s" % (
            B, row["lane_lane"]["viterbi_ms"]["median"], row["four_lane"]["viterbi_ms"]["median"], row["lane_lane"]["fic_ms"]["median"],
            row["lane_four"]["fic_ms"]["median"], row["lane_lane"]["ms_per_decode"]["median"], row["four_lane"]["ms_per_decode"]["median"],
            row["lane_four"]["ms_per_decode"]["median"], row["msc_four_wins"], row["fic_four_wins"]), file=sys.stderr)
    eng.close()
    msc_best = max([r["msc_groups"] for r in rows if r["msc_four_wins"]], default=0)
    fic_best = max([r["fic_tiles"] for r in rows if r["fic_four_wins"]], default=0)
    print(json.dumps({"what": "soft decisions at %.0f dB, IQ resident: the four-lane decoder against the lane form of the same build on the same box, rounds interleaved" % args.snr,
                      "snr_db": args.snr, "steps_per_round": args.steps, "rounds": args.rounds,
                      "rule": "four wins at a batch when its median is below the lane form's by more than the larger max - min spread of the two, for the stage and for the whole decode",
                      "curve": rows, "largest_winning_msc_groups": msc_best, "largest_winning_fic_tiles": fic_best}, indent=1))


if __name__ == "__main__":
    main()
