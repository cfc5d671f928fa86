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
    --trace-arm B --rounds 1     one arm only, for a separate kernel-trace run of the profiler

--windows: the encoder windows of include/css_mi355_session_window.h instead (float16, width = stride = 3000), arms H P W W0:
  H   run_enqueue_handoff x N, wait (arm B above): the floor
  P   the route without that header: H, then per session stream.session_windows in numpy and torch.from_numpy(...).cuda()
  W   run_enqueue_windows x N with the log-mel to the host as well, wait
  W0  the same with mel_host = NULL: no log-mel crosses PCIe
  W0n W0 with torch_sync=False: without the synchronise of torch's current stream before every enqueue
Windows of P, W and W0 are compared for bit equality.  --trace-arm W0 --rounds 1: one arm only, for a kernel-trace run.

--nemo: the hand-off to NeMo hosts of include/css_mi355_nemo_handoff.h (80 bands, the whole streams: drop_silence = 0, so that
every arm makes the features of the same samples), arms A B C D:
  A   the route without that header: run_enqueue x N, wait, then per stream the torch CPU rendering of the published definition
  B   run_enqueue_nemo x N with wav_host = NULL (features only), wait
  C   run_enqueue_handoff x N with wav_host = NULL (Whisper's features), wait: for scale
  D   the plain queue: run_enqueue x N, wait
B's features are compared with A's (float32 against float32: the largest difference is reported, not asserted)."""
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
    ap.add_argument("--trace-arm", default=None, choices=("P", "A", "B", "C", "D", "H", "W", "W0", "W0n"))
    ap.add_argument("--windows", action="store_true", help="the encoder-window arms H P W W0")
    ap.add_argument("--nemo", action="store_true", help="the NeMo hand-off arms A B C D")
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
    if a.windows:
        return window_arms(a, sep, run_cfg, pcm, n, n_out)
    if a.nemo:
        return nemo_arms(a, sep, run_cfg, pcm, n, n_out)
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


def window_arms(a, sep, run_cfg, pcm, n, n_out):
    import torch
    L, ST = pkg("_lib"), pkg("stream")
    h, desc, N = sep.handle, sep.desc, a.sessions
    S, nm, width = int(desc.num_spks), HANDOFF["n_mels"], 3000
    frames, ranges, nw = L.session_window_bounds(desc, run_cfg, L.handoff_cfg(**HANDOFF), width, width, n)
    wavs = {arm: [L.pinned_empty((S, n_out), np.float32) for _ in range(N)] for arm in ("H", "W", "W0", "W0n")}
    hos = {arm: [L.SessionHandoff(S, nm, frames, ranges) for _ in range(N)] for arm in ("H", "W", "W0", "W0n")}
    wins = {arm: [L.SessionWindows(0, S, nm, width, width, "float16", cap_windows=nw) for _ in range(N)] for arm in ("W", "W0", "W0n")}
    up_p = [None] * N

    def arm_h():
        for i in range(N):
            h.run_enqueue_handoff(pcm[i], run_cfg, wavs["H"][i], handoff=hos["H"][i], **HANDOFF)
        h.wait()

    def arm_p():
        arm_h()
        for i in range(N):
            ho, per = hos["H"][i], []
            for k in range(S):
                # (the host never learns M_k; the fill follows from the largest normalised value, (M + 4) / 4 -> M)
                mel = ho.mel[k]
                M = np.float32(mel.max()) * np.float32(4.0) - np.float32(4.0) if mel.shape[1] else np.float32(0)
                w = ST.session_windows(mel, M, width, width, "float16")
                per.append(np.concatenate([w, np.zeros((nw - w.shape[0], nm, width), np.float16)]))
            up_p[i] = torch.from_numpy(np.stack(per)).cuda()
        torch.cuda.synchronize()

    def arm_w(arm):
        for i in range(N):
            h.run_enqueue_windows(pcm[i], run_cfg, wavs[arm][i], width, width, "float16", mel_host=arm == "W", handoff=hos[arm][i],
                                  windows=wins[arm][i], torch_sync=arm != "W0n", **HANDOFF)
        h.wait()

    arms = {"H": arm_h, "P": arm_p, "W": lambda: arm_w("W"), "W0": lambda: arm_w("W0"), "W0n": lambda: arm_w("W0n")}
    order = [a.trace_arm] if a.trace_arm else ["H", "P", "W", "W0", "W0n"]
    for arm in order:
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
        equal = True
        for i in range(N):
            for k in range(S):
                nk = int(wins["W"][i].n_windows[k])
                ref = up_p[i][k, :nk].cpu().numpy()
                equal = equal and nk == int(wins["W0"][i].n_windows[k]) == -(-int(hos["H"][i].n_frames[k]) // width)
                got = {arm: wins[arm][i].windows[k, :nk].cpu().numpy() for arm in ("W", "W0", "W0n")}
                equal = equal and np.array_equal(got["W"], got["W0"]) and np.array_equal(got["W"], got["W0n"])
                for w in range(nk):   # (P's fill comes from a maximum recovered in float32: the frames are compared, not the padding)
                    nv = min(width, int(hos["H"][i].n_frames[k]) - w * width)
                    equal = equal and np.array_equal(got["W"][w, :, :nv], ref[w, :, :nv])
                equal = equal and np.array_equal(hos["W"][i].mel[k], hos["H"][i].mel[k])
            equal = equal and all(np.array_equal(wavs[arm][i], wavs["H"][i]) for arm in ("W", "W0", "W0n"))
    src = hos[order[-1] if order[-1] != "P" else "H"]
    mean_frames = float(np.mean([int(src[i].n_frames[k]) for i in range(N) for k in range(S)]))
    mean_windows = float(np.mean([-(-int(src[i].n_frames[k]) // width) for i in range(N) for k in range(S)]))
    up, wav_b, mel_b = n * 7 * 4, S * n_out * 4, S * nm * mean_frames * 4
    win_b = S * mean_windows * nm * width * 2
    small = S * (ranges * 16 + 12)
    out = dict(workload=f"{a.seconds:g} s x 7 channels, mc_v1, activity_th 0.3, {N} sessions per window, {a.rounds} windows per arm, "
                        f"{a.distinct} distinct recordings, hand-off {HANDOFF}, float16 windows of width = stride = {width}",
               ms_per_session={arm: dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)), all=[round(v, 4) for v in t])
                               for arm, t in times.items()},
               outputs_bit_equal=equal, mean_kept_frames_per_stream=mean_frames, mean_windows_per_stream=mean_windows,
               frame_bound=frames, window_bound=nw, window_bytes_written_per_session=win_b,
               pcie_bytes_per_session=dict(H=up + wav_b + mel_b + small, P=up + wav_b + mel_b + small + S * nw * nm * width * 2,
                                           W=up + wav_b + mel_b + small + S * 8, W0=up + wav_b + small + S * 8, W0n=up + wav_b + small + S * 8))
    if not a.trace_arm:
        med = {arm: out["ms_per_session"][arm]["median"] for arm in order}
        out["W0_minus_H_ms"] = med["W0"] - med["H"]
        out["W0n_minus_H_ms"] = med["W0n"] - med["H"]
        out["W_minus_H_ms"] = med["W"] - med["H"]
        out["P_minus_H_ms"] = med["P"] - med["H"]
        out["H_spread_ms"] = out["ms_per_session"]["H"]["max"] - out["ms_per_session"]["H"]["min"]
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    sep.close()


def nemo_arms(a, sep, run_cfg, pcm, n, n_out):
    import torch
    L, ST = pkg("_lib"), pkg("stream")
    h, desc, N = sep.handle, sep.desc, a.sessions
    S, nm = int(desc.num_spks), 80
    ncfg = dict(n_mels=nm, pad_frames=8, drop_silence=False, preemphasis=0.97, normalize=True)
    wcfg = dict(n_mels=nm, pad_frames=8, drop_silence=False)
    frames, ranges = L.nemo_handoff_bounds(desc, run_cfg, L.nemo_cfg(**ncfg), n)
    wavs = {arm: [L.pinned_empty((S, n_out), np.float32) for _ in range(N)] for arm in "AD"}
    nemo = [L.NemoHandoff(S, nm, frames, ranges) for _ in range(N)]
    whisper = [L.SessionHandoff(S, nm, frames, ranges) for _ in range(N)]
    bank = torch.from_numpy(ST.nemo_tables(nm)[1])
    window = torch.hann_window(400, periodic=False)
    feats_a = [None] * N

    def rendering(x):
        """the published class body (transformers' ParakeetFeatureExtractor) for one utterance, torch on the CPU, float32"""
        w = torch.from_numpy(x)[None, :]
        w = torch.cat([w[:, :1], w[:, 1:] - 0.97 * w[:, :-1]], dim=1)
        stft = torch.stft(w, 512, hop_length=160, win_length=400, window=window, return_complex=True, pad_mode="constant")
        mel = torch.log(bank @ torch.view_as_real(stft).pow(2).sum(-1) + 2 ** -24)[0, :, :x.shape[0] // 160]
        mean = mel.mean(dim=1, keepdim=True)
        std = torch.sqrt(((mel - mean) ** 2).sum(dim=1, keepdim=True) / (mel.shape[1] - 1))
        return ((mel - mean) / (std + 1e-5)).numpy()

    def arm_plain(out):
        for i in range(N):
            h.run_enqueue(pcm[i], run_cfg, out[i])
        h.wait()

    def arm_a():
        arm_plain(wavs["A"])
        for i in range(N):
            feats_a[i] = [rendering(wavs["A"][i][k]) for k in range(S)]

    def arm_b():
        for i in range(N):
            h.run_enqueue_nemo(pcm[i], run_cfg, None, handoff=nemo[i], **ncfg)
        h.wait()

    def arm_c():
        for i in range(N):
            h.run_enqueue_handoff(pcm[i], run_cfg, None, handoff=whisper[i], **wcfg)
        h.wait()

    arms = {"A": arm_a, "B": arm_b, "C": arm_c, "D": lambda: arm_plain(wavs["D"])}
    order = [a.trace_arm] if a.trace_arm else list("ABCD")
    for arm in order:                                        # warm-up: every buffer at its final size
        arms[arm]()
    times = {arm: [] for arm in order}
    for _ in range(a.rounds):
        for arm in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arms[arm]()
            times[arm].append((time.perf_counter() - t0) * 1e3 / N)
    diff = None
    if not a.trace_arm:
        diff = max(float(np.abs(nemo[i].mel[k] - feats_a[i][k]).max()) for i in range(N) for k in range(S))
        assert all(np.array_equal(wavs["A"][i], wavs["D"][i]) for i in range(N))
    up, wav_b, mel_b = n * 7 * 4, S * n_out * 4, S * nm * frames * 4
    out = dict(workload=f"{a.seconds:g} s x 7 channels, mc_v1, activity_th 0.3, {N} sessions per window, {a.rounds} windows per arm, "
                        f"{a.distinct} distinct recordings, NeMo hand-off {ncfg}",
               ms_per_session={arm: dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)), all=[round(v, 4) for v in t])
                               for arm, t in times.items()},
               max_abs_B_minus_A=diff, frames_per_stream=frames,
               pcie_bytes_per_session=dict(A=up + wav_b, B=up + mel_b, C=up + mel_b, D=up + wav_b))
    if not a.trace_arm:
        med = {arm: out["ms_per_session"][arm]["median"] for arm in order}
        out["B_minus_D_ms"] = med["B"] - med["D"]
        out["A_minus_D_ms"] = med["A"] - med["D"]
        out["C_minus_D_ms"] = med["C"] - med["D"]
        out["D_spread_ms"] = out["ms_per_session"]["D"]["max"] - out["ms_per_session"]["D"]["min"]
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    sep.close()


if __name__ == "__main__":
    main()
