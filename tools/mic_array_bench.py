"""What the MVDR kernels cost at each microphone count (csrc/mvdr.hip as a template over C).

    python tools/mic_array_bench.py [--rounds 9] [--out profiles/r23_mic_arrays.json]

One process, one model per C in {2, 4, 6, 7, 8} (one Conformer block: the estimator is not what is measured), one recording of 40
segments of 186 frames and 257 bins each (61.008 s).  Every round runs css_run once per C, the arms in turn, under the library's
own per-family event timing (css_set_profile: an event pair around each launch family; no profiler attached), and keeps the
covariance, solve and beamformer families.  Reported per C and family: the median, the smallest and the largest time over the
rounds, the number of launches, and the median divided by C = 7's median scaled by C^2 / 49 -- 1 where a kernel's cost follows the
packed matrix's size (the covariances; the solve is cubic in C, the beamformer linear: their ratios are read with that in mind)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAMILIES = ("scm", "mvdr_solve", "beamform")
CS = (2, 4, 6, 7, 8)
N_SAMPLES = (39 * 93 + 186) * 256          # 40 full segments of the shipped 3 s / 1.5 s segmentation


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_mic_arrays.json"))
    args = ap.parse_args()
    W = importlib.import_module("notsofar1_challenge_amd.weights")
    SYN = importlib.import_module("notsofar1_challenge_amd.synth")
    CSS = importlib.import_module("notsofar1_challenge_amd.css")
    SEP = importlib.import_module("notsofar1_challenge_amd.separator")
    cfg = CSS.CssCfg(activity_th=0.3, show_progressbar=False)
    arms = {}
    for C in CS:
        desc = W.ModelDesc(num_mics=C, in_features=257 * C, num_blocks=1)
        sep = SEP.HipSeparator(W.portable_state_dict(desc, 3), None, device=0, num_mics=C)
        x = np.ascontiguousarray(SYN.synth_meeting(N_SAMPLES / 16000.0 + 0.01, C, seed=8)[0, :N_SAMPLES])
        rc = CSS.make_run_cfg(cfg, 16000, C)
        h = sep.handle
        for _ in range(2):                  # warm-up: allocations, code objects, clocks
            h.run(x, rc)
        assert int(h.get_plan().num_segments) == 40
        arms[C] = (sep, h, x, rc)
    times = {C: {f: [] for f in FAMILIES} for C in CS}
    launches = {C: {} for C in CS}
    for _ in range(args.rounds):
        for C in CS:                        # the arms in turn inside every round
            _, h, x, rc = arms[C]
            h.set_profile(True)
            h.run(x, rc)
            ks = h.kernel_stats()
            h.set_profile(False)
            for f in FAMILIES:
                times[C][f].append(1e3 * ks[f][0])          # microseconds
                launches[C][f] = ks[f][1]
    for sep, *_ in arms.values():
        sep.close()
    med = {C: {f: float(np.median(times[C][f])) for f in FAMILIES} for C in CS}
    result = {"what": "covariance, solve and beamformer launches of 40 segments x 186 frames x 257 bins per microphone count C; "
                      "microseconds per css_run, medians over the rounds, arms alternated inside every round, event timing of the library",
              "rounds": args.rounds, "segments": 40, "frames": 186, "bins": 257, "per_C": {}}
    for C in CS:
        result["per_C"][str(C)] = {
            f: {"median_us": round(med[C][f], 2), "min_us": round(float(np.min(times[C][f])), 2), "max_us": round(float(np.max(times[C][f])), 2),
                "launches": int(launches[C][f]), "over_C7_scaled_by_C2_over_49": round(med[C][f] / (med[7][f] * C * C / 49.0), 3)}
            for f in FAMILIES}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
