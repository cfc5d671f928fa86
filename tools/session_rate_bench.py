#!/usr/bin/env python3
"""What a queue of 48 kHz sessions costs with both wav edges resampled on the device (include/css_mi355_session_rate.h), against the
routes that existed before: 60 s 7-channel 48 kHz PCM16 recordings, the 18-block model with the calibrated head, activity_th 0.3,
float32 mode, page-locked buffers.

Arms, alternated inside one process, the host clock around windows that end in css_wait (host passes included):
  A16  host scipy.signal.resample_poly to 16 kHz, int16 planes, run_enqueue_pcm16                      -> PCM16 streams at 16 kHz
  A48  host resample_poly to 16 kHz float32, run_enqueue, host resample_poly x 3, normalise, encode   -> PCM16 streams at 48 kHz
  B    Handle.resample (css_resample_host) to 16 kHz float32, run_enqueue                              -> float32 streams at 16 kHz
  C16  run_enqueue_pcm16_rate, 48 kHz in, 16 kHz out
  C48  run_enqueue_pcm16_rate, 48 kHz in and out
  D    the plain 16 kHz PCM16 queue (run_enqueue_pcm16), untouched by the rate calls
C16 is compared with write_wav's two lines on B's waveforms for bit equality at the size timed.

    python tools/session_rate_bench.py [--sessions 24] [--rounds 5] [--json OUT]
    --parent-tree DIR    a built checkout of the parent commit: arm D is also run there, in child processes that alternate with
                         child processes of this tree (--alternations each), so that D here is set against D there and against
                         the parent's own spread between its runs
    --root DIR --arms D  (what those child processes are given: the package is imported from DIR)"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("A16", "A48", "B", "C16", "C48", "D")


def stats(t):
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)), all=[round(float(v), 4) for v in t])


def encode(y):
    peaks = np.max(np.abs(y), axis=1).astype(np.float32)
    z = (y * np.float32(0.99)) / (peaks + np.float32(1e-7))[:, None]
    return np.clip(np.rint(z.astype(np.float64) * 32767.0), -32768.0, 32767.0).astype(np.int16)


def run_arms(a, root, arms):
    sys.path.insert(0, root)
    pkg = lambda n: importlib.import_module("notsofar1_challenge_amd." + n)
    import torch
    from scipy.signal import resample_poly
    W, SYN, CSS, SEP, L = pkg("weights"), pkg("synth"), pkg("css"), pkg("separator"), pkg("_lib")
    desc = W.ModelDesc.mc_v1()
    cal = np.load(os.path.join(root, "tests", "golden", "calib_mc.npz"))
    state = W.apply_golden_recipe(W.portable_state_dict(desc, 0), head_bias=cal["head_bias"])
    run_cfg = CSS.make_run_cfg(CSS.CssCfg(activity_th=0.3, show_progressbar=False), 16000, 7, desc.frame_len, desc.frame_hop)
    sep = SEP.HipSeparator(state, None, device=0, max_batch_segments=a.max_batch)
    h = sep.handle
    N, S = a.sessions, int(desc.num_spks)
    q16 = lambda x: np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)
    rate_arms = [m for m in arms if m != "D"]
    n16 = int(round(a.seconds * 16000))
    n_out16 = int(L.plan(desc, run_cfg, n16).n_out)
    planes16 = [L.pinned_copy(np.ascontiguousarray(q16(SYN.synth_meeting(a.seconds, 7, seed=1 + i)[0] * 0.1).T)) for i in range(a.distinct)]
    out = {}
    n_out48 = 0
    if rate_arms:
        planes48 = [L.pinned_copy(np.ascontiguousarray(q16(SYN.synth_meeting(a.seconds, 7, seed=11 + i, fs=48000)[0] * 0.1).T))
                    for i in range(a.distinct)]
        n48 = planes48[0].shape[1]
        r16, r48 = L.session_rate(48000, None), L.session_rate(48000, 48000)
        n_model, n_out_m, n_out48 = h.session_rate_samples(run_cfg, r48, n48)
        assert n_model == n16 and n_out_m == n_out16
        x16f = [L.pinned_empty((n16, 7), np.float32) for _ in range(N)]
        x16q = [L.pinned_empty((7, n16), np.int16) for _ in range(N)]
    o16 = {m: [L.pinned_empty((S, n_out16), np.int16) for _ in range(N)] for m in ("A16", "C16", "D") if m in arms}
    of = {m: [L.pinned_empty((S, n_out16), np.float32) for _ in range(N)] for m in ("A48", "B") if m in arms}
    o48 = {m: [L.pinned_empty((S, n_out48), np.int16) for _ in range(N)] for m in ("A48x", "C48") if m.rstrip("x") in arms}

    def arm_a16():
        for i in range(N):
            y = resample_poly(planes48[i % a.distinct].astype(np.float32) / np.float32(32768.0), 1, 3, axis=1)
            x16q[i][...] = q16(y)
            h.run_enqueue_pcm16([x16q[i][c] for c in range(7)], run_cfg, o16["A16"][i])
        h.wait()

    def arm_a48():
        for i in range(N):
            y = resample_poly(planes48[i % a.distinct].astype(np.float32) / np.float32(32768.0), 1, 3, axis=1)
            x16f[i][...] = y.T
            h.run_enqueue(x16f[i], run_cfg, of["A48"][i])
        h.wait()
        for i in range(N):
            o48["A48x"][i][...] = encode(resample_poly(of["A48"][i], 3, 1, axis=1).astype(np.float32)[:, :n_out48])

    def arm_b():
        for i in range(N):
            x16f[i][...] = h.resample(planes48[i % a.distinct].T, 48000)
            h.run_enqueue(x16f[i], run_cfg, of["B"][i])
        h.wait()

    def arm_c(rate, outs):
        for i in range(N):
            p = planes48[i % a.distinct]
            h.run_enqueue_pcm16_rate([p[c] for c in range(7)], run_cfg, rate, outs[i])
        h.wait()

    def arm_d():
        for i in range(N):
            p = planes16[i % a.distinct]
            h.run_enqueue_pcm16([p[c] for c in range(7)], run_cfg, o16["D"][i])
        h.wait()

    fns = {"A16": arm_a16, "A48": arm_a48, "B": arm_b, "C16": lambda: arm_c(r16, o16["C16"]), "C48": lambda: arm_c(r48, o48["C48"]),
           "D": arm_d}
    for m in arms:                                          # warm-up: every buffer at its final size
        fns[m]()
    times = {m: [] for m in arms}
    for _ in range(a.rounds):
        for m in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fns[m]()
            times[m].append((time.perf_counter() - t0) * 1e3 / N)
    out["ms_per_session"] = {m: stats(t) for m, t in times.items()}
    if "B" in arms and "C16" in arms:
        out["C16_equals_encoded_B"] = bool(all(np.array_equal(o16["C16"][i], encode(of["B"][i])) for i in range(N)))
    if rate_arms:
        out["pcie_bytes_per_session"] = dict(A16=7 * n16 * 2 + S * n_out16 * 2, A48=7 * n16 * 4 + S * n_out16 * 4,
                                             B=7 * n48 * 2 + 2 * 7 * n16 * 4 + S * n_out16 * 4, C16=7 * n48 * 2 + S * n_out16 * 2,
                                             C48=7 * n48 * 2 + S * n_out48 * 2, D=7 * n16 * 2 + S * n_out16 * 2)
    sep.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=24, help="sessions per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per arm")
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--distinct", type=int, default=2, help="distinct recordings the sessions cycle through")
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--arms", default=",".join(ALL))
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    arms = [m for m in a.arms.split(",") if m]
    assert all(m in ALL for m in arms), arms
    out = dict(workload=f"{a.seconds:g} s x 7 channels at 48 kHz PCM16 (D: 16 kHz), mc_v1, activity_th 0.3, float32 mode, {a.sessions} sessions "
                        f"per window, {a.rounds} windows per arm, {a.distinct} distinct recordings")
    out.update(run_arms(a, a.root, arms))
    if a.parent_tree:
        # arm D in fresh processes, this tree and the parent's alternating: D here against D there and the parent's own spread
        runs = {"this": [], "parent": []}
        for _ in range(a.alternations):
            for name, root in (("this", HERE), ("parent", a.parent_tree)):
                cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--arms", "D", "--sessions", str(a.sessions), "--rounds",
                       str(a.rounds), "--seconds", str(a.seconds), "--distinct", str(a.distinct), "--max-batch", str(a.max_batch)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError(f"arm D in {root} ended with {r.returncode}: {r.stderr[-2000:]}")
                runs[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_session"]["D"]["median"])
        med = {k: float(np.median(v)) for k, v in runs.items()}
        out["D_processes"] = dict(medians_ms_per_session=runs, this=med["this"], parent=med["parent"],
                                  parent_spread_ms=float(max(runs["parent"]) - min(runs["parent"])),
                                  this_minus_parent_ms=med["this"] - med["parent"],
                                  within_parent_spread=bool(abs(med["this"] - med["parent"]) <= max(runs["parent"]) - min(runs["parent"])))
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
