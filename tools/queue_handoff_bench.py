#!/usr/bin/env python3
"""What the hand-off to Whisper costs a queue of sessions (include/css_mi355_session_handoff.h), on bench.py's own workload: the
60 s 7-channel meeting, the 18-block model with the calibrated head, activity_th 0.3, page-locked buffers.

Arms, alternated inside one process (P A B C P A B C ...), the host clock around windows that end in css_wait:
  P  the plain queue: run_enqueue x N, wait
  A  the only route to log-mel without this header: P, then per session run_device + three css_handoff_logmel calls
  B  run_enqueue_handoff x N with waveforms, wait
  C  the same with wav_host = NULL (log-mel only)
Every arm's outputs are compared for bit equality at the sizes timed (waveforms of P, A, B; log-mel and ranges of A, B, C).

    python tools/queue_handoff_bench.py [--sessions 24] [--rounds 5] [--json OUT]
    --trace-arm B --rounds 1     one arm only, for a separate kernel-trace run of the profiler"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = lambda n: importlib.import_module("notsofar1_challenge_amd." + n)
HANDOFF = dict(n_mels=80, pad_frames=8, drop_silence=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=24, help="sessions per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per arm")
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--distinct", type=int, default=4, help="distinct recordings the sessions cycle through")
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--trace-arm", default=None, choices=("P", "A", "B", "C"))
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    W, SYN, CSS, SEP, L = pkg("weights"), pkg("synth"), pkg("css"), pkg("separator"), pkg("_lib")
    desc = W.ModelDesc.mc_v1()
    cal = np.load(os.path.join(ROOT, "tests", "golden", "calib_mc.npz"))
    state = W.apply_golden_recipe(W.portable_state_dict(desc, 0), head_bias=cal["head_bias"])
    run_cfg = CSS.make_run_cfg(CSS.CssCfg(activity_th=0.3, show_progressbar=False), 16000, 7, desc.frame_len, desc.frame_hop)
    sep = SEP.HipSeparator(state, None, device=0, max_batch_segments=a.max_batch)
    h = sep.handle
    N, S, nm = a.sessions, int(desc.num_spks), HANDOFF["n_mels"]
    recs = [L.pinned_copy(np.ascontiguousarray(SYN.synth_meeting(a.seconds, 7, seed=1 + i)[0])) for i in range(a.distinct)]
    n = recs[0].shape[0]
    n_out = int(L.plan(desc, run_cfg, n).n_out)
    frames, ranges = L.session_handoff_bounds(desc, run_cfg, L.handoff_cfg(**HANDOFF), n)
    pcm = [recs[i % a.distinct] for i in range(N)]
    wavs = {arm: [L.pinned_empty((S, n_out), np.float32) for _ in range(N)] for arm in "PAB"}
    hos = {arm: [L.SessionHandoff(S, nm, frames, ranges) for _ in range(N)] for arm in "BC"}
    dev_pcm = [torch.from_numpy(np.asarray(r)).cuda() for r in recs]
    dev_wav = torch.empty((S, n_out), dtype=torch.float32, device="cuda")
    res_a = [None] * N

    def arm_p(out):
        for i in range(N):
            h.run_enqueue(pcm[i], run_cfg, out[i])
        h.wait()

    def arm_a():
        arm_p(wavs["A"])
        for i in range(N):
            h.run_device(dev_pcm[i % a.distinct].data_ptr(), n, 7, run_cfg, dev_wav.data_ptr(), n_out)
            res_a[i] = [h.handoff_logmel(dev_wav.data_ptr(), n_out, k, **HANDOFF) for k in range(S)]

    def arm_bc(arm):
        for i in range(N):
            h.run_enqueue_handoff(pcm[i], run_cfg, wavs["B"][i] if arm == "B" else None, handoff=hos[arm][i], **HANDOFF)
        h.wait()

    arms = {"P": lambda: arm_p(wavs["P"]), "A": arm_a, "B": lambda: arm_bc("B"), "C": lambda: arm_bc("C")}
    order = [a.trace_arm] if a.trace_arm else list("PABC")
    for arm in order:                                        # warm-up: every buffer at its final size
        arms[arm]()
    times = {arm: [] for arm in order}
    for _ in range(a.rounds):
        for arm in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arms[arm]()
            times[arm].append((time.perf_counter() - t0) * 1e3 / N)
    equal = None
    if not a.trace_arm:
        equal = all(np.array_equal(wavs["P"][i], wavs["A"][i]) and np.array_equal(wavs["P"][i], wavs["B"][i]) for i in range(N))
        for i in range(N):
            for k in range(S):
                mel, reg = res_a[i][k]
                for arm in "BC":
                    equal = equal and np.array_equal(hos[arm][i].mel[k], mel) and np.array_equal(hos[arm][i].ranges[k], reg)
    src = "C" if not a.trace_arm else (a.trace_arm if a.trace_arm in "BC" else None)
    mean_frames = float(np.mean([int(hos[src][i].n_frames[k]) for i in range(N) for k in range(S)])) if src else None
    up, wav_b = n * 7 * 4, S * n_out * 4
    mel_b = None if mean_frames is None else S * nm * mean_frames * 4
    out = dict(workload=f"{a.seconds:g} s x 7 channels, mc_v1, activity_th 0.3, {N} sessions per window, {a.rounds} windows per arm, "
                        f"{a.distinct} distinct recordings, hand-off {HANDOFF}",
               ms_per_session={arm: dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)), all=[round(v, 4) for v in t])
                               for arm, t in times.items()},
               outputs_bit_equal=equal, mean_kept_frames_per_stream=mean_frames, frame_bound=frames, range_bound=ranges,
               pcie_bytes_per_session=dict(P=up + wav_b, A=None if mel_b is None else up + wav_b + mel_b + S * (n_out // 256 - 1),
                                           B=None if mel_b is None else up + wav_b + mel_b, C=None if mel_b is None else up + mel_b))
    if not a.trace_arm:
        med = {arm: out["ms_per_session"][arm]["median"] for arm in "PABC"}
        out["B_over_A"] = med["B"] / med["A"]
        out["B_minus_P_ms"] = med["B"] - med["P"]
        out["C_minus_P_ms"] = med["C"] - med["P"]
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    sep.close()


if __name__ == "__main__":
    main()
