"""Streaming separation on one MI355X: per-push wall time (host clock around the synchronous push, which ends in its
device-to-host copy), aggregate real-time factor, observed lag, device memory per stream, and css_run on the same input
in the same process for context.  Prints one JSON document (profiles/r07_stream_bench.json holds a run).

    python tools/stream_bench.py [--minutes 1 10] [--pushes 0.5 1.5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FS = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, nargs="+", default=[1.0, 10.0])
    ap.add_argument("--pushes", type=float, nargs="+", default=[0.5, 1.5])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import notsofar1_challenge_amd.css as CSS
    import notsofar1_challenge_amd.separator as SEP
    import notsofar1_challenge_amd.stream as STR
    import notsofar1_challenge_amd.synth as SYN
    import notsofar1_challenge_amd.weights as W
    desc = W.ModelDesc.mc_v1()
    st = W.apply_golden_recipe(W.portable_state_dict(desc, 0))
    sep = SEP.HipSeparator(st, None, device=0, max_batch_segments=256)
    cfg = CSS.CssCfg()
    rc = CSS.make_run_cfg(cfg, FS, 7)
    res = {"model": "mc_v1 (18 blocks, exact float32)", "cfg": "3 s / 1.5 s segments, defaults", "runs": []}
    for minutes in a.minutes:
        x = SYN.synth_meeting(60.0 * minutes, 7, seed=1)[0]
        x = np.ascontiguousarray(x)
        sep.handle.run(x[:FS * 10], rc)   # warm-up
        t0 = time.perf_counter()
        ref = sep.handle.run(x, rc).copy()
        t_run = time.perf_counter() - t0
        for push_s in a.pushes:
            step = int(push_s * FS)
            times, lags = [], []
            with STR.CssStream(sep, cfg) as s:
                s.push(x[:step])   # warm-up of this stream's first kernels
                outs = []
                s.close()
            with STR.CssStream(sep, cfg) as s:
                outs = []
                total0 = time.perf_counter()
                for i in range(0, x.shape[0], step):
                    t = time.perf_counter()
                    outs.append(np.stack(s.push(x[i:i + step])))
                    times.append(time.perf_counter() - t)
                    inf = s.info()
                    lags.append((inf.n_pushed - inf.n_emitted) / FS)
                outs.append(np.stack(s.finish()))
                total = time.perf_counter() - total0
                dev = s.info().device_bytes
                lag_bound = s.latency_samples / FS
            same = bool(np.array_equal(np.concatenate(outs, 1), ref))
            ms = np.array(times) * 1e3
            res["runs"].append({
                "meeting_s": 60.0 * minutes, "push_s": push_s, "pushes": len(times),
                "push_ms_p50": round(float(np.percentile(ms, 50)), 3), "push_ms_p99": round(float(np.percentile(ms, 99)), 3),
                "push_ms_max": round(float(ms.max()), 3),
                "stream_rtf_x": round(60.0 * minutes / total, 1),
                "lag_s_median": round(float(np.median(lags)), 3), "lag_s_max": round(float(max(lags)), 3), "lag_bound_s": lag_bound,
                "device_bytes": int(dev), "bit_identical_to_css_run": same,
                "css_run_s": round(t_run, 4), "css_run_rtf_x": round(60.0 * minutes / t_run, 1)})
            print(json.dumps(res["runs"][-1]), flush=True)
    sep.close()
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
