#!/usr/bin/env python3
"""A queue of sessions on one GPU (css_run_enqueue / css_wait): every session goes from float PCM in page-locked host
memory to separated waveforms in page-locked host memory; a session's PCIe legs run under its neighbours' kernels, and
consecutive sessions share mask-estimator batches (up to max_batch_segments segments per batch).

    python examples/session_queue.py [n_sessions] [--logmel [--windows]] [--nemo]

--logmel: every session also hands Whisper its input (css_run_enqueue_handoff): the kept sample ranges and the normalised
log-mel of each separated stream, computed on the GPU behind the session's waveforms; one session takes no waveforms at all.
--windows (with --logmel): the log-mel never leaves the GPU (css_run_enqueue_windows with mel_host = NULL): every session leaves
Whisper's float16 encoder inputs [S, windows, 80, 3000] and the whole padded log-mel for seek-based decoding in torch tensors.
--nemo: every session hands a NeMo host its input instead (css_run_enqueue_nemo): the kept ranges and NeMo's log-mel features
(pre-emphasis 0.97, symmetric Hann in a 512-point transform, ln(x + 2^-24), per-band normalisation) of each separated stream."""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
pkg = lambda n: importlib.import_module("notsofar1_challenge_amd." + n)
css, _lib, sepmod, weights, synth = (pkg(n) for n in ("css", "_lib", "separator", "weights", "synth"))

logmel, windows, nemo = "--logmel" in sys.argv[1:], "--windows" in sys.argv[1:], "--nemo" in sys.argv[1:]
args = [a for a in sys.argv[1:] if a not in ("--logmel", "--windows", "--nemo")]
n_sessions = int(args[0]) if args else 8
desc = weights.ModelDesc.mc_v1()                                     # a real deployment: separator.load_css_model(dir)
state = weights.apply_golden_recipe(weights.portable_state_dict(desc, 0))
sep = sepmod.HipSeparator(state, None, device=0, max_batch_segments=128)
h = sep.handle
run_cfg = css.make_run_cfg(css.CssCfg(activity_th=0.3, show_progressbar=False), 16000, 7)

# sessions of different lengths; inputs and outputs in page-locked memory (css_host_alloc)
sessions = []
for k in range(n_sessions):
    pcm = _lib.pinned_copy(np.ascontiguousarray(synth.synth_meeting(40.0 + 10.0 * (k % 4), 7, seed=k)[0]))
    plan = _lib.plan(desc, run_cfg, pcm.shape[0])
    sessions.append((pcm, _lib.pinned_empty((3, int(plan.n_out)), np.float32)))
h.run(max((p for p, _ in sessions), key=lambda p: p.shape[0]), run_cfg)   # warm-up: buffers sized for the longest session
for pcm, out in sessions:                                            # ... and one untimed queue: the handle allocates the
    h.run_enqueue(pcm, run_cfg, out)                                 # per-session buffers of a shared batch on first use
h.wait()

t0 = time.perf_counter()
views = [h.run_enqueue(pcm, run_cfg, out) for pcm, out in sessions]  # returns at once
h.wait()                                                             # every `out` is valid now
queued = time.perf_counter() - t0
t0 = time.perf_counter()
refs = [h.run(pcm, run_cfg).copy() for pcm, _ in sessions]           # the same sessions, one synchronous call each
sync = time.perf_counter() - t0
audio = sum(p.shape[0] for p, _ in sessions) / 16000.0
print(f"{n_sessions} sessions, {audio:.0f} s of 7-channel audio: queued {1e3 * queued:.1f} ms ({audio / queued:.0f} x real time), "
      f"one call per session {1e3 * sync:.1f} ms ({audio / sync:.0f} x real time); same bits: "
      f"{all(np.array_equal(v, r) for v, r in zip(views, refs))}")
if logmel and windows:
    import torch
    torch.zeros(1, device="cuda")                                    # (torch's own start-up on the GPU stays out of the timing)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = [h.run_enqueue_windows(pcm, run_cfg, None if k == 0 else out, width=3000, stride=3000, dtype="float16", mel_host=False, seek=True)
           for k, (pcm, out) in enumerate(sessions)]
    h.wait()                                                         # waveforms, ranges, counts and the tensors are valid now
    handed = time.perf_counter() - t0
    for k, (view, ho, win) in enumerate(got[:3]):
        for spk in range(3):
            n = int(win.n_windows[spk])                              # encoder inputs win.windows[spk, :n]; win.mel[spk][:, seek:seek + 3000]
            print(f"  session {k} stream {spk}: {int(ho.n_frames[spk])} frames in {n} windows {tuple(win.windows[spk, :n].shape)} "
                  f"{win.windows.dtype}, on {win.windows.device}; clamp at {float(win.window_max[spk]):.3f}")
    print(f"with encoder windows on the device: {1e3 * handed:.1f} ms ({audio / handed:.0f} x real time); waveforms the same bits: "
          f"{all(np.array_equal(v, r) for (v, _, _), r in list(zip(got, refs))[1:])}")
elif logmel:
    t0 = time.perf_counter()
    got = [h.run_enqueue_handoff(pcm, run_cfg, None if k == 0 else out, n_mels=80, pad_frames=8, drop_silence=True)
           for k, (pcm, out) in enumerate(sessions)]
    h.wait()                                                         # waveforms, ranges and log-mel are valid now
    handed = time.perf_counter() - t0
    for k, (view, ho) in enumerate(got[:3]):
        for spk in range(3):
            r = ho.ranges[spk]                                       # [n, 2] sample ranges of the meeting, in order: the time map
            kept = int((r[:, 1] - r[:, 0]).sum())                    # frame j of ho.mel[spk] starts at concatenated sample 160 j
            print(f"  session {k} stream {spk}: {len(r)} ranges, {kept / 16000.0:.1f} s kept, log-mel {ho.mel[spk].shape}")
    print(f"with the hand-off: {1e3 * handed:.1f} ms ({audio / handed:.0f} x real time); waveforms the same bits: "
          f"{all(np.array_equal(v, r) for (v, _), r in list(zip(got, refs))[1:])}")
if nemo:
    t0 = time.perf_counter()
    got = [h.run_enqueue_nemo(pcm, run_cfg, None if k == 0 else out, n_mels=80, pad_frames=8, drop_silence=True, preemphasis=0.97,
                              normalize=True) for k, (pcm, out) in enumerate(sessions)]
    h.wait()                                                         # waveforms, ranges, features and statistics are valid now
    handed = time.perf_counter() - t0
    for k, (view, ho) in enumerate(got[:3]):
        for spk in range(3):
            r = ho.ranges[spk]                                       # frame j of ho.mel[spk] is centred on concatenated sample 160 j
            print(f"  session {k} stream {spk}: {len(r)} ranges, features {ho.mel[spk].shape}, "
                  f"raw mean {float(ho.mean[spk].mean()):.2f}" if int(ho.n_frames[spk]) else f"  session {k} stream {spk}: silent")
    print(f"with the NeMo hand-off: {1e3 * handed:.1f} ms ({audio / handed:.0f} x real time); waveforms the same bits: "
          f"{all(np.array_equal(v, r) for (v, _), r in list(zip(got, refs))[1:])}")
if os.environ.get("DEBUG"):
    for k, (v, r) in enumerate(zip(views, refs)):
        bad = np.flatnonzero((v != r).any(axis=0))
        print(k, v.shape, "equal" if bad.size == 0 else f"{bad.size} samples differ, first {bad[0]}, last {bad[-1]}, max {np.abs(v - r).max():.3e}")
sep.close()
