"""What tools/bench_coco_eval.py and tools/bench_lvis_eval.py share for `--accumulate both`: the evaluator's device path on the whole set
with the accumulation in numpy and on the device, in ONE run on the same packed arrays, so that the numpy tail is the yardstick of the
device tail.  The tails: numpy = the `tail` lap (accumulate_arrays + summarize; the `copy_out` of match, ignore and rank that feeds it is
shown beside it); device = accumulate + copy_out (precision and recall) + tail (summarize).  Laps are the host clock after a device
synchronise (vid_eval._Laps)."""
import statistics

import numpy as np

LAPS = ("copy_in", "kernel", "accumulate", "copy_out", "tail")


def compare(module, packed, num_classes, device, repeats, warmup, what):
    """module: coco_eval or lvis_eval; packed: evaluate_device's positional arguments -> the record's lines"""
    res, med, spread = {}, {}, {}
    for mode in ("numpy", "device"):
        runs = []
        for i in range(warmup + repeats):
            times = {}
            res[mode] = module.evaluate_device(*packed, num_classes, device=device, times=times, accumulate=mode)
            if i >= warmup:
                runs.append(times)
            print("  accumulate=%s run %d: %s" % (mode, i, " ".join("%s %.3f" % (k, times[k]) for k in LAPS if k in times)), flush=True)
        med[mode] = {k: statistics.median(r.get(k, 0.0) for r in runs) for k in LAPS}
        tails = [r["tail"] if mode == "numpy" else r["accumulate"] + r["copy_out"] + r["tail"] for r in runs]
        spread[mode] = (statistics.median(tails), min(tails), max(tails))
    same = {k: bool(np.array_equal(res["numpy"][k], res["device"][k])) for k in ("precision", "recall", "stats")}
    text = module.result_string(res["numpy"]["stats"]) == module.result_string(res["device"]["stats"])
    n, d = med["numpy"], med["device"]
    return ["",
            "  %s, accumulation in numpy and on the device, whole set, medians of %d after %d warm-up" % (what, repeats, warmup),
            "    numpy   tail %.3f s (min %.3f max %.3f) = accumulate_arrays + summarize; in front of it: kernel %.3f s, copy_out %.3f s "
            "(match, ignore, rank, dets)" % (spread["numpy"] + (n["kernel"], n["copy_out"])),
            "    device  tail %.3f s (min %.3f max %.3f) = accumulate %.4f + copy_out %.4f (precision, recall) + summarize %.4f; in front of it: "
            "kernel %.3f s" % (spread["device"] + (d["accumulate"], d["copy_out"], d["tail"], d["kernel"])),
            "    the device tail is %.1fx shorter than the numpy tail" % (spread["numpy"][0] / spread["device"][0]) if spread["device"][0] < spread["numpy"][0]
            else "    the device tail is NOT shorter than the numpy tail",
            "    precision %s, recall %s, stats %s, text %s" % tuple("identical" if v else "DIFFERENT" for v in (same["precision"], same["recall"],
                                                                                                          same["stats"], text))]
