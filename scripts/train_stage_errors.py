"""Merge the figure files tests/test_gpu_train_stages.py writes (WW_TRAIN_STAGE_JSON, one per pytest run) into
profiles/train_stage_errors.json and print the worst ratio error / allowance per stage (the table in DESIGN.md).

    WW_TRAIN_STAGE_JSON=a.json pytest -m gpu tests/test_gpu_train_stages.py -k "not benchmark_batch"
    WW_TRAIN_STAGE_JSON=b.json pytest -m gpu tests/test_gpu_train_stages.py -k benchmark_batch
    python scripts/train_stage_errors.py a.json b.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(paths):
    figures = [f for p in paths for f in json.load(open(p))]
    worst = {}
    for f in figures:
        for stage, v in f.get("ratios", {}).items():
            key = (f["kind"], stage)
            if key not in worst or v > worst[key][0]:
                worst[key] = (v, f"{f['arch']} {f['train_math']} batch {f['batch']} width {f['width']}")
    summary = {f"{kind}:{stage}": {"worst_ratio": v, "case": case} for (kind, stage), (v, case) in sorted(worst.items())}
    with open(os.path.join(ROOT, "profiles", "train_stage_errors.json"), "w") as out:
        json.dump({"worst_per_stage": summary, "whole_step": [f for f in figures if f["kind"] == "whole_step"],
                   "cases": [f for f in figures if f["kind"] != "whole_step"]}, out, indent=1)
    for name, e in summary.items():
        print(f"{name:24s} {e['worst_ratio']:.3f}   {e['case']}")
    for f in figures:
        if f["kind"] == "whole_step":
            print(f"whole step {f['arch']} batch {f['batch']}: float64 replays {f['replay_seconds'][0]:.1f} s / {f['replay_seconds'][1]:.1f} s")


if __name__ == "__main__":
    main(sys.argv[1:])
