"""Streaming separation on one MI355X: per-push wall time (host clock around the synchronous push, which ends in its
device-to-host copy), aggregate real-time factor, observed lag, device memory per stream, and css_run on the same input
in the same process for context.  Prints one JSON document (profiles/r07_stream_bench.json holds a run).

    python tools/stream_bench.py [--minutes 1 10] [--pushes 0.5 1.5] [--out FILE]

With --streams N: N live meetings of 60 s fed in rounds of 1.5 s per stream, two arms on the same streams in alternating
blocks of rounds (so that clock and power state are shared): (A) N css_stream_push calls per round, one after the other;
(B) one css_stream_push_many per round.  A stream's output does not depend on the arm that pushed a round, so both arms
work on ONE set of streams; every returned piece is compared with css_run's output for the recording.  Per arm: p50 / p99 ms
per round, streams served in real time per GPU (1.5 s / round time x N), bit_identical (profiles/r09_stream_group.json).

    python tools/stream_bench.py --streams 16 [--out FILE]

With --handoff every stream has the hand-off to the ASR front end switched on (80 bands, pad 8, drop silence): the rounds
then also return log-mel frames, kept ranges and gate bits (profiles/r10_stream_handoff.json).  --only-grouped runs arm B alone.

With --pcm16 the recordings are 16-bit PCM (quantised at 0.2 of full scale) and the arms that alternate are B, fed the
dequantised float32 samples, and (C) one css_stream_push_many_pcm16 per round on the int16 samples themselves, interleaved
as a capture device delivers them (--pinned: in page-locked memory).  Every arm's input is laid out before the clock starts;
every arm is compared with css_run of the dequantised recording (profiles/r11_stream_pcm16.json).

With --rate HZ the recordings are 16-bit PCM at HZ (the synthetic meeting interpolated to that rate) and the streams are opened
with input_rate=HZ: one arm, (R) one css_stream_push_many_pcm16 per round of 1.5 s at HZ, resampled to 16 kHz by the ingest
kernel; compared with css_run of Handle.resample of the recording (--pinned as above; profiles/r12_stream_rate.json).

With --preview arm B runs alone and every round is followed by (P) one css_stream_preview_many of all streams, timed on its own;
at three rounds of a pass every stream's preview is compared with css_run of the samples pushed so far, outside the clock
(profiles/r13_stream_preview.json).  --passes sets the timed passes over the recordings (default 2).

With --handoff --preview a third call follows: (PH) one css_stream_preview_handoff_many of all streams, timed on its own; at the
same three rounds every stream's provisional frames, ranges and gate bits, with what its pushes returned so far, are compared
with css_run_device + css_handoff_logmel of the samples pushed so far, outside the clock (profiles/r14_stream_preview_handoff.json).

With --handoff --window arm B runs alone on streams opened with window_history=3000 and, from the first round after which every
separated stream holds a frame, two calls follow each round, timed on their own: (W) one css_stream_windows for 3 float16 windows
of width 3000 per stream (the last frames of every separated stream) into one torch tensor on the device, and (H) what a host
does today with the same frames, which it has accumulated from the pushes' hand-offs outside the clock: numpy whisper_normalize
over the span, pad, cast to float16 and torch.from_numpy(...).cuda().  At three rounds both are compared, outside the clock
(profiles/r15_stream_window.json).  --handoff --history opens the streams with the same history and runs arm B alone: what the
history costs a round, without the two calls between the rounds.

With --handoff --preview --window everything above runs in every round and one more call follows, timed on its own: (PW) one
css_stream_present_windows of all streams -- arm PH's preview and arm W's 3 float16 windows of width 3000 per stream in one call
and under one synchronise, the windows reaching over the preview's provisional frames to the present.  PH, W and PW follow one
another inside every round, so they share clock and power state; at three rounds PW's windows are compared with whisper_window of
the host's frames followed by the preview's, outside the clock (profiles/r16_stream_present_window.json).

With --rate HZ --out-rate HZ2 [--out-pcm16] two groups of N streams take the same 16-bit recordings at HZ, one round of 1.5 s each
per tick, in an order that alternates in blocks of rounds: (O) one css_stream_push_many_pcm16 on streams opened with
output=dict(rate=HZ2, dtype=int16 or float32) and no model-rate out_host: the final samples come back at HZ2, converted on the
device; (F) the same push on streams without an output format, followed by what a host does today with the float32 samples it
gets: scipy.signal.resample_poly to HZ2 and, with --out-pcm16, the rounding to int16, per separated stream.  Arm O is compared
with the definition (css_resample_host of css_run's waveforms, _lib.pcm16_encode), arm F's float32 samples with css_run; the
bytes that cross PCIe per tick are counted for both (profiles/r20_stream_output.json).

With --nemo (with --streams) four arms run, each in a fresh process of its own and alternated: the plain grouped tick, the same
with the Whisper hand-off, with the NeMo hand-off (CssStream(nemo=...), include/css_mi355_stream_nemo.h), and the host's route --
the plain tick, then stream.nemo_features of every returned piece on the CPU.  --parent-library PATH adds the plain and the
Whisper arm on an earlier build of the library, between this one's (profiles/r27_stream_nemo.json).

With --nemo --chunks three arms run the same way: the NeMo tick on the earlier build (--parent-library), on this one without a
frame history and with one of 3000 frames (CssStream(nemo_history=3000), include/css_mi355_nemo_chunk.h).  Behind its last pass the
third arm times one CssStreamGroup.nemo_chunks call of 48 per-feature float16 chunks, of 400 frames and of up to 3000, against the
host's route for the same chunks: numpy's per-feature normalisation of the frames the pushes returned, stacked, cast and uploaded
with torch.from_numpy(...).cuda(); the device's chunks are first compared with stream.nemo_chunk_features, bit for bit
(profiles/r28_stream_nemo_chunks.json).  --repeats sets how often every arm runs.
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


HANDOFF = dict(n_mels=80, pad_frames=8, drop_silence=True)


def group_bench(n_streams, out_path, seconds=60.0, round_s=1.5, block=5, passes=2, handoff=False, only_grouped=False, pcm16=False,
                pinned=False, rate=0, preview=False, window=False, history=False):
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
    recs = [np.ascontiguousarray(SYN.synth_meeting(seconds, 7, seed=1000 + i)[0]) for i in range(n_streams)]
    q16 = []
    if rate:
        import notsofar1_challenge_amd._lib as LIB
        t = np.arange(int(round(seconds * rate))) * (float(FS) / rate)
        at = np.arange(recs[0].shape[0])
        q16 = [np.clip(np.rint(np.stack([np.interp(t, at, x[:, c]) for c in range(7)], axis=1) * 0.2 * 32768.0), -32768, 32767).astype(np.int16)
               for x in recs]
        recs = [sep.handle.resample(q, rate) for q in q16]
        if pinned:
            q16 = [LIB.pinned_copy(q) for q in q16]
    elif pcm16:
        import notsofar1_challenge_amd._lib as LIB
        q16 = [np.clip(np.rint(x.astype(np.float64) * 0.2 * 32768.0), -32768, 32767).astype(np.int16) for x in recs]
        recs = [np.ascontiguousarray(q.astype(np.float32) / np.float32(32768.0)) for q in q16]
        if pinned:
            q16 = [LIB.pinned_copy(q) for q in q16]
    sep.handle.run(recs[0][:FS * 10], rc)   # warm-up
    refs = [sep.handle.run(x, rc).copy() for x in recs]
    step = int(round_s * (rate or FS))
    arms = "RR" if rate else ("BC" if pcm16 else "AB")
    only_grouped = only_grouped or preview or window or history
    ms = {"A": [], "B": [], "C": [], "R": [], "P": [], "PH": [], "W": [], "H": [], "PW": []}
    same = {"A": True, "B": True, "C": True, "R": True, "P": True, "PH": True, "W": True, "H": True, "PW": True}
    present = preview and handoff and window
    present_launches, present_provisional, present_checks, pw_rounds = [], [], [], []
    window_bytes, window_frames, window_launches, window_checks = [], [], [], []
    WIDTH = 3000
    preview_frames = []
    preview_checks, preview_samples, preview_segments = [], [], []
    seg_per_batch = []
    mel_frames = []

    def prefix_handoff_equal(x, calls, pv_wav, pv):
        """pushes' hand-offs + the preview's against css_run_device + css_handoff_logmel of the prefix x"""
        import torch
        import notsofar1_challenge_amd._lib as LIB
        h = sep.handle
        n_out = int(LIB.plan(desc, rc, x.shape[0]).n_out)
        pcm = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        wav = torch.empty((3, n_out), dtype=torch.float32, device="cuda")
        h.run_device(pcm.data_ptr(), x.shape[0], 7, rc, wav.data_ptr(), n_out)
        torch.cuda.synchronize()
        act = h.read(LIB.BUF_ACT_FINAL).copy()
        ok = bool(np.array_equal(pv_wav, wav.cpu().numpy()[:, n_out - pv_wav.shape[1]:]))
        for k in range(3):
            mel, regions = h.handoff_logmel(wav.data_ptr(), n_out, k, **HANDOFF)
            merged = []
            for lo, hi in np.concatenate([c.ranges[k] for c in calls] + [pv.ranges[k]]):
                if merged and lo <= merged[-1][1]:
                    merged[-1][1] = max(merged[-1][1], int(hi))
                else:
                    merged.append([int(lo), int(hi)])
            raw = np.concatenate([c.mel[k] for c in calls] + [pv.mel[k]], axis=1)
            ok = ok and bool(np.array_equal(np.array(merged, np.int64).reshape(-1, 2), regions))
            ok = ok and bool(np.array_equal(np.concatenate([c.activity[k] for c in calls] + [pv.activity[k]]), act[k]))
            ok = ok and pv.first_frame[k] == sum(c.mel[k].shape[1] for c in calls)
            ok = ok and bool(np.array_equal(STR.whisper_normalize(raw, pv.raw_max[k]), mel))
        return ok

    def one_pass(first_arm, timed):
        streams = [STR.CssStream(sep, cfg, handoff=HANDOFF if handoff else None, input_rate=rate or None,
                                 window_history=WIDTH if window or history else None) for _ in recs]
        group = STR.CssStreamGroup(streams)
        raw = [[np.zeros((HANDOFF["n_mels"], 0), np.float32) for _ in range(3)] for _ in recs]   # (arm H: the host's own history)
        if window:
            import torch
            w_out = torch.empty((3 * n_streams, HANDOFF["n_mels"], WIDTH), dtype=torch.float16, device="cuda")
            pw_out = torch.empty_like(w_out) if present else None
        em = [0] * n_streams
        calls = [[] for _ in recs]   # (arm PH: every push's hand-off, for the comparison with the offline call)
        n_rounds = ((q16 if rate else recs)[0].shape[0] + step - 1) // step if timed else 2 * block
        for r in range(n_rounds):
            arm = "B" if only_grouped else arms[(r // block + (first_arm == arms[1])) % 2]
            chunks = [x[r * step:(r + 1) * step] for x in (q16 if arm in "CR" else recs)]
            t = time.perf_counter()
            if arm == "A":
                res = [s.push(c) for s, c in zip(streams, chunks)]
            elif arm in "CR":
                res = group.push_pcm16(chunks)
            else:
                res = group.push(chunks)
            dt = time.perf_counter() - t
            batches, segments = group.stats.estimator_batches, group.stats.estimator_segments
            if preview:
                t = time.perf_counter()
                pv = group.preview()
                dt_p = time.perf_counter() - t
                if timed:
                    ms["P"].append(dt_p * 1e3)
                    preview_segments.append(group.stats.estimator_segments / max(group.stats.estimator_batches, 1))
                    preview_samples.append(float(np.median([p[0].shape[0] for p in pv if p is not None] or [0])))
                    if r in (n_rounds // 8, n_rounds // 2, n_rounds - 2):   # css_run of every prefix, outside the clock
                        for i, p in enumerate(pv):
                            n = min((r + 1) * step, recs[i].shape[0])
                            want = sep.handle.run(recs[i][:n], rc)[:, em[i] + res[i][0].shape[0]:]
                            same["P"] = same["P"] and p is not None and bool(np.array_equal(np.stack(p), want))
                        preview_checks.append(r)
            if preview and handoff:
                for i, s in enumerate(streams):
                    calls[i].append(s.handoff)
                t = time.perf_counter()
                pvh = group.preview(handoff=True)
                dt_ph = time.perf_counter() - t
                if timed:
                    ms["PH"].append(dt_ph * 1e3)
                    preview_frames.append(float(np.median([sum(m.shape[1] for m in s.preview_handoff.mel) for s in streams
                                                           if s.preview_handoff is not None] or [0])))
                    if r in (n_rounds // 8, n_rounds // 2, n_rounds - 2):   # the offline hand-off of every prefix, outside the clock
                        for i, p in enumerate(pvh):
                            n = min((r + 1) * step, recs[i].shape[0])
                            same["PH"] = same["PH"] and p is not None and streams[i].preview_handoff is not None and \
                                prefix_handoff_equal(recs[i][:n], calls[i], np.stack(p), streams[i].preview_handoff)
            if window:
                for i, s in enumerate(streams):
                    raw[i] = [np.concatenate([a, m], axis=1)[:, -WIDTH:] for a, m in zip(raw[i], s.handoff.mel)]
                if all(a.shape[1] > 0 for r_ in raw for a in r_):
                    reqs = [(s, k) for s in streams for k in range(3)]
                    t = time.perf_counter()
                    group.windows(reqs, width=WIDTH, dtype="float16", out=w_out)
                    dt_w = time.perf_counter() - t
                    t = time.perf_counter()
                    host = np.stack([STR.whisper_window(a, WIDTH, "float16") for r_ in raw for a in r_])
                    up = torch.from_numpy(host).cuda()
                    torch.cuda.synchronize()
                    dt_h = time.perf_counter() - t
                    if timed:
                        ms["W"].append(dt_w * 1e3)
                        ms["H"].append(dt_h * 1e3)
                        nm = HANDOFF["n_mels"]
                        frames = [a.shape[1] for r_ in raw for a in r_]
                        window_frames.append(float(np.median(frames)))
                        window_bytes.append(sum(f * (nm + 1) * 4 for f in frames) + len(frames) * nm * WIDTH * 2)
                        window_launches.append(group.window_launches)
                        if r in (n_rounds // 8, n_rounds // 2, n_rounds - 2):   # outside the clock
                            same["W"] = same["W"] and bool(np.array_equal(w_out.cpu().numpy(), host))
                            same["H"] = same["H"] and bool(torch.equal(up, w_out))
                            window_checks.append(r)
                    if present:
                        t = time.perf_counter()
                        _, spans, _ = group.present_windows(reqs, width=WIDTH, dtype="float16", out=pw_out)
                        dt_pw = time.perf_counter() - t
                        if timed:
                            ms["PW"].append(dt_pw * 1e3)
                            pw_rounds.append((dt_ph * 1e3, dt_w * 1e3, dt_pw * 1e3))
                            present_launches.append(group.window_launches)
                            present_provisional.append(float(np.median(spans[:, 2])))
                            if r in (n_rounds // 8, n_rounds // 2, n_rounds - 2):   # outside the clock
                                want = np.stack([STR.whisper_window(np.concatenate([a, s.preview_handoff.mel[k]], axis=1)[:, -WIDTH:], WIDTH, "float16")
                                                 for s, r_ in zip(streams, raw) for k, a in enumerate(r_)])
                                same["PW"] = same["PW"] and bool(np.array_equal(pw_out.cpu().numpy(), want))
                                present_checks.append(r)
            if not timed:
                continue
            ms[arm].append(dt * 1e3)
            if arm != "A" and batches:
                seg_per_batch.append(segments / batches)
            if handoff:
                mel_frames.append(sum(m.shape[1] for s in streams for m in s.handoff.mel))
            for i, got in enumerate(res):
                got = np.stack(got)
                same[arm] = same[arm] and bool(np.array_equal(got, refs[i][:, em[i]:em[i] + got.shape[1]]))
                em[i] += got.shape[1]
        if timed:
            for i, s in enumerate(streams):
                got = np.stack(s.finish())
                ok = bool(np.array_equal(got, refs[i][:, em[i]:])) and em[i] + got.shape[1] == refs[i].shape[1]
                for a in same:
                    same[a] = same[a] and ok
        dev = streams[0].info().device_bytes
        for s in streams:
            s.close()
        return dev

    one_pass(arms[0], False)   # warm-up: both arms, segments included
    dev = 0
    for p in range(passes):
        dev = one_pass(arms[p % 2], True)
    res = {"model": "mc_v1 (18 blocks, exact float32)", "cfg": "3 s / 1.5 s segments, defaults", "streams": n_streams,
           "meeting_s": seconds, "round_s": round_s, "block_rounds": block, "device_bytes_per_stream": int(dev),
           "segments_per_estimator_batch_median": float(np.median(seg_per_batch)) if seg_per_batch else 0.0, "arms": {}}
    if handoff:
        res["window_history_frames"] = WIDTH if window or history else 0
        res["handoff"] = dict(HANDOFF, mel_frames_per_round_median=float(np.median(mel_frames)),
                              launches_products_frames_last_call=list(sep.handle.stream_handoff_stats()))
    if rate:
        res["input"] = "16-bit PCM at %d Hz, 0.2 of full scale (%s); the streams resample to %d Hz at ingest" % (
            rate, "page-locked" if pinned else "pageable", FS)
    elif pcm16:
        res["input"] = "16-bit PCM at 0.2 of full scale; arm B is fed the dequantised float32 samples, arm C the int16 samples (%s)" % (
            "page-locked" if pinned else "pageable")
    if preview:
        res["preview"] = {"rounds_compared_with_css_run_of_the_prefix": preview_checks,
                          "samples_per_stream_median": float(np.median(preview_samples)) if preview_samples else 0.0,
                          "segments_per_estimator_batch_median": float(np.median(preview_segments)) if preview_segments else 0.0}
        if handoff:
            res["preview"]["handoff_mel_frames_per_stream_median"] = float(np.median(preview_frames)) if preview_frames else 0.0
    if window and ms["W"]:
        w50 = float(np.percentile(np.array(ms["W"]), 50))
        # bytes the windows need (frames and their maxima read, windows written) over the wall time of the whole CALL -- checks,
        # launches, the download of the maxima, the synchronise -- per round; the kernel's own rate needs a kernel trace
        rate = [b / (m * 1e-3) for b, m in zip(window_bytes, ms["W"])]
        res["window"] = {"windows_per_call": 3 * n_streams, "width": WIDTH, "dtype": "float16", "history_frames": WIDTH,
                         "launches_per_call": int(max(window_launches)), "rounds_compared": window_checks,
                         "frames_per_window_median": float(np.median(window_frames)),
                         "bytes_per_call_median": float(np.median(window_bytes)), "bytes_per_call_mean": float(np.mean(window_bytes)),
                         "calls": len(window_bytes),
                         "frames_per_window_max": float(max(window_frames)),
                         "call_GB_per_s_median": round(float(np.median(rate)) * 1e-9, 2),
                         "call_GB_per_s_last_round": round(rate[-1] * 1e-9, 2),
                         "p50_ratio_H_over_W": round(float(np.percentile(np.array(ms["H"]), 50)) / w50, 3)}
    if present and ms["PW"]:
        v = np.array(pw_rounds)   # [rounds, (PH, W, PW)] of the rounds that ran all three
        p50 = [float(np.percentile(v[:, i], 50)) for i in range(3)]
        res["present_window"] = {"windows_per_call": 3 * n_streams, "width": WIDTH, "dtype": "float16", "history_frames": WIDTH,
                                 "launches_per_call": int(max(present_launches)), "rounds_compared": present_checks,
                                 "provisional_frames_per_window_median": float(np.median(present_provisional)),
                                 "rounds_with_PH_W_and_PW": int(v.shape[0]),
                                 "PH_ms_p50_same_rounds": round(p50[0], 3), "W_ms_p50_same_rounds": round(p50[1], 3),
                                 "PW_ms_p50": round(p50[2], 3),
                                 "PW_minus_PH_plus_W_ms_p50_of_rounds": round(float(np.percentile(v[:, 2] - v[:, 0] - v[:, 1], 50)), 3),
                                 "PW_minus_PH_plus_W_ms_p10_p90_of_rounds": [round(float(np.percentile(v[:, 2] - v[:, 0] - v[:, 1], q)), 3) for q in (10, 90)]}
    for arm, what in (("A", "one css_stream_push per stream and round"), ("B", "one css_stream_push_many per round"),
                      ("P", "one css_stream_preview_many per round, after arm B's push"),
                      ("PH", "one css_stream_preview_handoff_many per round, after arm P's preview"),
                      ("W", "one css_stream_windows per round: 3 float16 windows of width 3000 per stream, on the device"),
                      ("H", "the same windows by numpy whisper_window of the host's frames + torch.from_numpy(...).cuda()"),
                      ("PW", "one css_stream_present_windows per round: arm PH's preview and arm W's windows, up to the present, in one call"),
                      ("C", "one css_stream_push_many_pcm16 per round"),
                      ("R", "one css_stream_push_many_pcm16 per round, streams opened with input_rate")):
        if not ms[arm]:
            continue
        v = np.array(ms[arm])
        p50 = float(np.percentile(v, 50))
        res["arms"][arm] = {"what": what, "rounds": int(v.size), "round_ms_p50": round(p50, 3),
                            "round_ms_p99": round(float(np.percentile(v, 99)), 3),
                            "streams_in_real_time_per_gpu": round(round_s * 1e3 / p50 * n_streams, 1), "bit_identical": same[arm]}
    if "C" in res["arms"]:
        res["p50_ratio_C_over_B"] = round(res["arms"]["C"]["round_ms_p50"] / res["arms"]["B"]["round_ms_p50"], 4)
    if "P" in res["arms"]:
        res["arms"]["P"].pop("streams_in_real_time_per_gpu")
        res["p50_ratio_P_over_B"] = round(res["arms"]["P"]["round_ms_p50"] / res["arms"]["B"]["round_ms_p50"], 4)
    for arm in ("W", "H", "PW"):
        if arm in res["arms"]:
            res["arms"][arm].pop("streams_in_real_time_per_gpu")
    if "PH" in res["arms"]:
        res["arms"]["PH"].pop("streams_in_real_time_per_gpu")
        res["p50_ratio_PH_over_P"] = round(res["arms"]["PH"]["round_ms_p50"] / res["arms"]["P"]["round_ms_p50"], 4)
    if "A" in res["arms"]:
        res["p50_ratio_B_over_A"] = round(res["arms"]["B"]["round_ms_p50"] / res["arms"]["A"]["round_ms_p50"], 4)
    sep.close()
    text = json.dumps(res, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(text)


NEMO = dict(n_mels=80, pad_frames=8, drop_silence=True, preemphasis=0.97)
NEMO_ARMS = {"plain": "one css_stream_push_many per tick, no hand-off",
             "whisper": "the same, every stream with the Whisper hand-off (80 bands, pad 8, drop silence)",
             "nemo": "the same, every stream with the NeMo hand-off (80 bands, pad 8, drop silence, p = 0.97)",
             "host": "the plain tick, then the raw NeMo features of every returned piece on the CPU (numpy float32 on BLAS: host_nemo_features)",
             "history": "the NeMo tick, every stream with a frame history of 3000 frames (nemo_history=3000); behind the last pass, one "
                        "nemo_chunks call of 48 per-feature float16 chunks against the host's route for the same chunks"}
CHUNK_HISTORY = 3000


def chunk_calls(group, streams, kept, repeats=20):
    """--nemo --chunks, behind the timed ticks: (b) one CssStreamGroup.nemo_chunks call of 48 per-feature float16 chunks and (c) the
    host's route for the same chunks -- numpy's per-feature normalisation of the frames the pushes returned (`kept`), stacked and
    uploaded into a torch tensor -- for spans of 400 frames and of up to 3000; every timed call is first checked bit-identical to
    stream.nemo_chunk_features.  -> {n_frames: {...}}"""
    import torch
    import notsofar1_challenge_amd.stream as STR
    out = {}
    # the 48 (stream, speaker) pairs that hold the most frames; a span is as long as the shortest of them allows
    pairs = sorted(((kept[i][k].shape[1], i, k) for i in range(len(streams)) for k in range(3)), reverse=True)[:48]
    for want in (400, 3000):
        n = min(want, pairs[-1][0], CHUNK_HISTORY)
        if n < 1:
            continue
        reqs = [(streams[i], k) for _, i, k in pairs]
        spans = [kept[streams.index(s)][k][:, -n:] for s, k in reqs]
        buf = torch.empty((len(reqs), NEMO["n_mels"], n), dtype=torch.float16, device="cuda")
        got = group.nemo_chunks([(s, k, None, n) for s, k in reqs], n, "per_feature", "float16", 0.0, out=buf).cpu().numpy()
        same = all(np.array_equal(got[i].view(np.uint16), STR.nemo_chunk_features(spans[i], n, "per_feature", "float16").view(np.uint16))
                   for i in range(len(reqs)))
        if not same:   # (no timing of a call that does not give the statement's bits)
            raise SystemExit(f"nemo_chunks of {n} frames differs from stream.nemo_chunk_features: nothing is timed")
        dev, host = [], []
        for _ in range(repeats):
            t = time.perf_counter()
            group.nemo_chunks([(s, k, None, n) for s, k in reqs], n, "per_feature", "float16", 0.0, out=buf)
            dev.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            batch = np.stack(spans)
            mean = batch.mean(axis=2, dtype=np.float64)
            std = np.sqrt(((batch - mean[:, :, None]) ** 2).sum(axis=2) / max(n - 1, 1))
            norm = ((batch - mean.astype(np.float32)[:, :, None]) / (std.astype(np.float32)[:, :, None] + np.float32(1e-5))).astype(np.float16)
            up = torch.from_numpy(norm).cuda()
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t) * 1e3)
        close = float(np.abs(up.cpu().numpy().astype(np.float32) - got.astype(np.float32)).max())
        out[str(want)] = {"n_frames": n, "chunks": len(reqs), "launches": group.window_launches, "bit_identical_to_numpy_statement": bool(same),
                          "device_call_ms_median": round(float(np.median(dev)), 4), "device_call_ms_min": round(min(dev), 4),
                          "host_route_ms_median": round(float(np.median(host)), 4), "host_route_ms_min": round(min(host), 4),
                          "host_route_max_abs_difference": close}
    return out


def host_nemo_features(tables, x, p):
    """what a host computes per returned piece: stream.nemo_features(x, normalize=False)'s arithmetic with the frames laid out
    contiguously, so that both products run on BLAS (the package's own statement multiplies a strided view)"""
    A, Wm = tables
    L = len(x) // 160
    if L == 0:
        return np.zeros((Wm.shape[0], 0), np.float32)
    y = x.copy()
    if p:
        y[1:] = x[1:] - np.float32(p) * x[:-1]
    padded = np.concatenate([np.zeros(256, np.float32), y, np.zeros(256, np.float32)])
    frames = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(padded, 512)[::160][:L].T)
    spec = A @ frames
    power = spec[:257] * spec[:257] + spec[257:] * spec[257:]
    return np.log(Wm @ power + np.float32(2.0 ** -24))


def nemo_arm(arm, n_streams, seconds=60.0, round_s=1.5, passes=2):
    """One arm of --nemo in this process (the library is CSS_MI355_LIBRARY's, or the tree's): a warm-up pass, then `passes` timed
    passes of grouped ticks over `n_streams` meetings; prints one JSON line {"arm", "tick_ms": [...], "bit_identical", ...}."""
    import notsofar1_challenge_amd._lib as LIB
    if os.environ.get("CSS_MI355_LIBRARY"):
        # (an earlier build of the library: the entries it does not export yet are taken out of the binding; no arm on it asks for one)
        import ctypes
        LIB._share_hip_runtime_with_torch()
        probe = ctypes.CDLL(LIB.LIB_PATH)
        for table in (LIB.STREAM_NEMO_ABI, LIB.NEMO_CHUNK_ABI):
            for name in [n for n in table if not hasattr(probe, n)]:
                del table[name]
    import notsofar1_challenge_amd.css as CSS
    import notsofar1_challenge_amd.separator as SEP
    import notsofar1_challenge_amd.stream as STR
    import notsofar1_challenge_amd.synth as SYN
    import notsofar1_challenge_amd.weights as W
    desc = W.ModelDesc.mc_v1()
    sep = SEP.HipSeparator(W.apply_golden_recipe(W.portable_state_dict(desc, 0)), None, device=0, max_batch_segments=256)
    cfg = CSS.CssCfg()
    rc = CSS.make_run_cfg(cfg, FS, 7)
    recs = [np.ascontiguousarray(SYN.synth_meeting(seconds, 7, seed=1000 + i)[0]) for i in range(n_streams)]
    sep.handle.run(recs[0][:FS * 10], rc)   # warm-up
    refs = [sep.handle.run(x, rc).copy() for x in recs]
    step = int(round_s * FS)
    tables = STR.nemo_tables(NEMO["n_mels"])
    ms, same, frames, chunk_res = [], True, [], None
    for p in range(passes + 1):
        kw = {"whisper": dict(handoff=HANDOFF), "nemo": dict(nemo=NEMO), "history": dict(nemo=NEMO, nemo_history=CHUNK_HISTORY)}.get(arm, {})
        kept = [[np.zeros((NEMO["n_mels"], 0), np.float32) for _ in range(3)] for _ in recs]   # (the host's own history, for the host's route)
        streams = [STR.CssStream(sep, cfg, **kw) for _ in recs]
        group = STR.CssStreamGroup(streams)
        em = [0] * n_streams
        for r in range((recs[0].shape[0] + step - 1) // step):
            chunks = [x[r * step:(r + 1) * step] for x in recs]
            t = time.perf_counter()
            res = group.push(chunks)
            if arm == "host":
                feats = [host_nemo_features(tables, w, NEMO["preemphasis"]) for got in res for w in got]
            dt = time.perf_counter() - t
            if p > 0:
                ms.append(dt * 1e3)
                if arm == "host":
                    frames.append(sum(f.shape[1] for f in feats))
                elif arm != "plain":
                    frames.append(sum(m.shape[1] for s in streams for m in (s.handoff if arm == "whisper" else s.nemo).mel))
            if arm == "history" and p == passes:
                kept = [[np.concatenate([kept[i][k], s.nemo.mel[k]], axis=1)[:, -CHUNK_HISTORY:] for k in range(3)] for i, s in enumerate(streams)]
            for i, got in enumerate(res):
                got = np.stack(got)
                same = same and bool(np.array_equal(got, refs[i][:, em[i]:em[i] + got.shape[1]]))
                em[i] += got.shape[1]
        if arm == "history" and p == passes:
            chunk_res = chunk_calls(group, streams, kept)
        for i, s in enumerate(streams):
            got = np.stack(s.finish())
            same = same and bool(np.array_equal(got, refs[i][:, em[i]:])) and em[i] + got.shape[1] == refs[i].shape[1]
            s.close()
    stats = list(sep.handle.stream_handoff_stats())
    sep.close()
    print("NEMO_ARM " + json.dumps({"arm": arm, "library": os.environ.get("CSS_MI355_LIBRARY") or "this", "tick_ms": [round(v, 4) for v in ms],
                                    "bit_identical": same, "frames_per_tick_median": float(np.median(frames)) if frames else 0.0,
                                    "launches_products_frames_last_call": stats, "chunks": chunk_res}))


def nemo_bench(n_streams, out_path, parent_library, repeats=3, passes=2, chunks=False):
    """--nemo: every arm in a fresh process of its own, one after the other and alternated -- the parent commit's library (plain,
    Whisper) between this commit's arms -- `repeats` times; per arm the tick's p50 of every repeat, their median [min, max].
    chunks (--nemo --chunks): the NeMo tick on the parent's library, on this one without a history and with one, and the chunk calls
    the `history` arm times behind its last pass (profiles/r28_stream_nemo_chunks.json)."""
    import subprocess
    order = [("plain", True), ("plain", False), ("whisper", True), ("whisper", False), ("nemo", False), ("host", False)]
    if chunks:
        order = [("nemo", True), ("nemo", False), ("history", False)]
    if not parent_library:
        order = [o for o in order if not o[1]]
    got = {}
    for rep in range(repeats):
        for arm, parent in (order if rep % 2 == 0 else order[::-1]):
            env = dict(os.environ)
            env.pop("CSS_MI355_LIBRARY", None)
            if parent:
                env["CSS_MI355_LIBRARY"] = os.path.abspath(parent_library)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--nemo-arm", arm, "--streams", str(n_streams), "--passes", str(passes)],
                                 env=env, capture_output=True, text=True, timeout=900)
            if out.returncode != 0:   # (a child that failed ends the measurement: nothing more is started on the GPU)
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                raise SystemExit(f"arm {arm} ({'parent' if parent else 'this'}) ended with {out.returncode}")
            print(f"repeat {rep}: arm {arm} ({'parent' if parent else 'this'}) done", file=sys.stderr, flush=True)
            line = [l for l in out.stdout.splitlines() if l.startswith("NEMO_ARM ")][-1]
            got.setdefault(("parent " if parent else "this ") + arm, []).append(json.loads(line[len("NEMO_ARM "):]))
    res = {"what": "tools/stream_bench.py --nemo --streams %d: 60 s meetings, mc_v1 (18 blocks, exact float32), 1.5 s grouped ticks, every arm in a "
                   "process of its own, arms alternated in one job, %d repeats of %d timed passes" % (n_streams, repeats, passes),
           "hand-offs": {"whisper": HANDOFF, "nemo": NEMO}, "arms": {}}
    for name, runs in got.items():
        p50 = [float(np.percentile(np.array(r["tick_ms"]), 50)) for r in runs]
        res["arms"][name] = {"what": NEMO_ARMS[name.split()[1]], "tick_ms_p50_per_repeat": [round(v, 3) for v in p50],
                             "tick_ms_median": round(float(np.median(p50)), 3), "tick_ms_min": round(min(p50), 3), "tick_ms_max": round(max(p50), 3),
                             "ticks_per_repeat": len(runs[0]["tick_ms"]), "bit_identical": all(r["bit_identical"] for r in runs),
                             "frames_per_tick_median": runs[0]["frames_per_tick_median"],
                             "launches_products_frames_last_call": runs[0]["launches_products_frames_last_call"]}
        if any(r.get("chunks") for r in runs):
            res["arms"][name]["chunk_calls_per_repeat"] = [r["chunks"] for r in runs]
    a = res["arms"]
    med = lambda k: a[k]["tick_ms_median"]
    if chunks:
        res["what"] = res["what"].replace("--nemo ", "--nemo --chunks ")
        res["history_minus_no_history_ms"] = round(med("this history") - med("this nemo"), 3)
        if parent_library:
            pr = a["parent nemo"]
            spread = pr["tick_ms_max"] - pr["tick_ms_min"]
            res["parent_nemo_spread_ms"] = round(spread, 3)
            res["bar_for_history_ms"] = round(pr["tick_ms_median"] + spread + 0.03 * pr["tick_ms_median"], 3)
            res["history_within_bar"] = bool(med("this history") <= res["bar_for_history_ms"])
            res["this_minus_parent_nemo_ms"] = round(med("this nemo") - pr["tick_ms_median"], 3)
    else:
        res["extra_over_plain_ms"] = {k: round(med("this " + k) - med("this plain"), 3) for k in ("whisper", "nemo", "host")}
    if parent_library and not chunks:
        for k in ("plain", "whisper"):
            pr = a["parent " + k]
            res["this_minus_parent_" + k + "_ms"] = round(med("this " + k) - med("parent " + k), 3)
            res["parent_" + k + "_spread_ms"] = round(pr["tick_ms_max"] - pr["tick_ms_min"], 3)
    text = json.dumps(res, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(text)


def output_bench(n_streams, out_path, rate, out_rate, out_pcm16, pinned=False, seconds=60.0, round_s=1.5, block=5, passes=2):
    from scipy.signal import resample_poly
    import notsofar1_challenge_amd._lib as LIB
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
    recs = [np.ascontiguousarray(SYN.synth_meeting(seconds, 7, seed=1000 + i)[0]) for i in range(n_streams)]
    t = np.arange(int(round(seconds * rate))) * (float(FS) / rate)
    at = np.arange(recs[0].shape[0])
    q16 = [np.clip(np.rint(np.stack([np.interp(t, at, x[:, c]) for c in range(7)], axis=1) * 0.2 * 32768.0), -32768, 32767).astype(np.int16)
           for x in recs]
    recs = [sep.handle.resample(q, rate) if rate != FS else np.ascontiguousarray(q.astype(np.float32) / np.float32(32768.0)) for q in q16]
    if pinned:
        q16 = [LIB.pinned_copy(q) for q in q16]
    sep.handle.run(recs[0][:FS * 10], rc)   # warm-up
    refs = [sep.handle.run(x, rc).copy() for x in recs]
    gain = 1.0
    ocfg = LIB.stream_output_cfg(out_rate, "int16" if out_pcm16 else "float32", gain)
    up, down = ocfg.up, ocfg.down

    def definition(w):
        y = w if up == down else np.ascontiguousarray(sep.handle.resample(w.T, FS, out_rate).T)
        return np.stack([LIB.pcm16_encode(v, gain)[0] for v in y]) if out_pcm16 else y
    want = [definition(w) for w in refs]
    step = int(round_s * rate)
    ms = {"O": [], "F": [], "F_push": []}
    same = {"O": True, "F": True}
    worst = 0.0   # arm F against the definition: float64 taps and sums against the float32 chain
    launches = []

    def host_convert(res):
        out = []
        for per_stream in res:
            y = [v if up == down else resample_poly(v, up, down) for v in per_stream]
            out.append([np.clip(np.rint(v.astype(np.float64) * gain * 32767.0), -32768, 32767).astype(np.int16) for v in y] if out_pcm16 else y)
        return out

    def one_pass(first, timed):
        so = [STR.CssStream(sep, cfg, input_rate=rate if rate != FS else None,
                            output=dict(rate=out_rate, dtype="int16" if out_pcm16 else "float32", gain=gain)) for _ in recs]
        sf = [STR.CssStream(sep, cfg, input_rate=rate if rate != FS else None) for _ in recs]
        go, gf = STR.CssStreamGroup(so), STR.CssStreamGroup(sf)
        emo, emf = [0] * n_streams, [0] * n_streams
        n_rounds = (q16[0].shape[0] + step - 1) // step if timed else 2 * block
        for r in range(n_rounds):
            chunks = [q[r * step:(r + 1) * step] for q in q16]
            order = "OF" if (r // block + (first == "F")) % 2 == 0 else "FO"
            for arm in order:
                t0 = time.perf_counter()
                if arm == "O":
                    res_o = go.push_pcm16(chunks)
                    dt = time.perf_counter() - t0
                    launches.append(sep.handle.stream_output_stats())
                else:
                    res_f = gf.push_pcm16(chunks)
                    dt_push = time.perf_counter() - t0
                    conv = host_convert(res_f)
                    dt = time.perf_counter() - t0
                if timed:
                    ms[arm].append(dt * 1e3)
                    if arm == "F":
                        ms["F_push"].append(dt_push * 1e3)
            if not timed:
                continue
            for i in range(n_streams):
                got = np.stack(res_o[i])
                same["O"] = same["O"] and bool(np.array_equal(got, want[i][:, emo[i]:emo[i] + got.shape[1]]))
                emo[i] += got.shape[1]
                gf_ = np.stack(res_f[i])
                same["F"] = same["F"] and bool(np.array_equal(gf_, refs[i][:, emf[i]:emf[i] + gf_.shape[1]]))
                emf[i] += gf_.shape[1]
        if timed:
            for i in range(n_streams):
                got = np.stack(so[i].finish())
                same["O"] = same["O"] and bool(np.array_equal(got, want[i][:, emo[i]:])) and emo[i] + got.shape[1] == want[i].shape[1]
                sf[i].finish()
        dev = (so[0].info().device_bytes, sf[0].info().device_bytes)
        for s in so + sf:
            s.close()
        return dev

    one_pass("O", False)
    dev = (0, 0)
    for p in range(passes):
        dev = one_pass("OF"[p % 2], True)
    # one whole recording through the host's route, against the definition (in output LSB for int16, else absolute)
    whole = host_convert([list(refs[0])])[0]
    worst = float(np.abs(np.stack(whole).astype(np.float64) - want[0].astype(np.float64)).max())
    per_tick_in = n_streams * step * 7 * 2
    spk = 3 * n_streams
    res = {"model": "mc_v1 (18 blocks, exact float32)", "cfg": "3 s / 1.5 s segments, defaults", "streams": n_streams, "meeting_s": seconds,
           "round_s": round_s, "block_rounds": block, "passes": passes,
           "input": "16-bit PCM at %d Hz, 0.2 of full scale (%s)" % (rate, "page-locked" if pinned else "pageable"),
           "output": "%s at %d Hz, gain %g" % ("int16" if out_pcm16 else "float32", out_rate, gain),
           "device_bytes_per_stream": {"O": int(dev[0]), "F": int(dev[1])},
           "output_kernel_launches_and_rounds_per_call_max": [int(max(a for a, _ in launches)), int(max(b for _, b in launches))],
           "pcie_bytes_per_tick": {"O": {"in": per_tick_in, "out": int(spk * round_s * out_rate * (2 if out_pcm16 else 4))},
                                   "F": {"in": per_tick_in, "out": int(spk * round_s * FS * 4)}},
           "host_route_max_abs_difference_from_the_definition": worst, "arms": {}}
    for arm, what in (("O", "one css_stream_push_many_pcm16 per tick, streams with the output format, no model-rate out_host"),
                      ("F", "the same push on streams without an output format + scipy.signal.resample_poly%s on the host for %d speaker streams"
                       % (" and the int16 conversion" if out_pcm16 else "", spk)),
                      ("F_push", "arm F's push alone")):
        v = np.array(ms[arm])
        res["arms"][arm] = {"what": what, "ticks": int(v.size), "tick_ms_p50": round(float(np.percentile(v, 50)), 3),
                            "tick_ms_p10": round(float(np.percentile(v, 10)), 3), "tick_ms_p90": round(float(np.percentile(v, 90)), 3),
                            "tick_ms_p99": round(float(np.percentile(v, 99)), 3)}
        if arm in same:
            res["arms"][arm]["bit_identical"] = same[arm]
    res["p50_ratio_O_over_F"] = round(res["arms"]["O"]["tick_ms_p50"] / res["arms"]["F"]["tick_ms_p50"], 4)
    sep.close()
    text = json.dumps(res, indent=1)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, nargs="+", default=[1.0, 10.0])
    ap.add_argument("--pushes", type=float, nargs="+", default=[0.5, 1.5])
    ap.add_argument("--streams", type=int, default=0, help="grouped pushes: N live meetings, per-stream pushes against one grouped push per round")
    ap.add_argument("--handoff", action="store_true", help="with --streams: every stream returns log-mel frames, kept ranges and gate bits")
    ap.add_argument("--only-grouped", action="store_true", help="with --streams: arm B alone (twice the rounds)")
    ap.add_argument("--pcm16", action="store_true", help="with --streams: arms B (float32) and C (css_stream_push_many_pcm16) on 16-bit recordings")
    ap.add_argument("--pinned", action="store_true", help="with --pcm16: arm C's int16 samples in page-locked memory")
    ap.add_argument("--rate", type=int, default=0, help="with --streams: 16-bit recordings at this rate, streams opened with input_rate (arm R alone)")
    ap.add_argument("--preview", action="store_true", help="with --streams: arm B alone, each round followed by one css_stream_preview_many (arm P) and, with --handoff, "
                    "one css_stream_preview_handoff_many (arm PH)")
    ap.add_argument("--window", action="store_true", help="with --streams --handoff: streams keep a 3000-frame history; arm B alone, each round followed by one "
                    "css_stream_windows (arm W) and the host's route to the same windows (arm H); with --preview also one "
                    "css_stream_present_windows (arm PW)")
    ap.add_argument("--history", action="store_true", help="with --streams --handoff: streams keep a 3000-frame history; arm B alone")
    ap.add_argument("--out-rate", type=int, default=0, help="with --streams --rate: arm O, streams with the output format at this rate, against arm F, "
                    "plain streams + scipy.signal.resample_poly on the host")
    ap.add_argument("--out-pcm16", action="store_true", help="with --out-rate: the output is int16 (the host's route converts too)")
    ap.add_argument("--passes", type=int, default=2, help="with --streams: timed passes over the recordings")
    ap.add_argument("--nemo", action="store_true", help="with --streams: plain, Whisper hand-off, NeMo hand-off and the host's route, each arm in a process "
                    "of its own, alternated (profiles/r27_stream_nemo.json)")
    ap.add_argument("--chunks", action="store_true", help="with --nemo: the NeMo tick on the parent's library, without and with a frame history, and one "
                    "nemo_chunks call of 48 chunks against the host's route (profiles/r28_stream_nemo_chunks.json)")
    ap.add_argument("--repeats", type=int, default=3, help="with --nemo: how often every arm runs")
    ap.add_argument("--parent-library", default=None, help="with --nemo: an earlier build of the library; its arms run between this one's")
    ap.add_argument("--nemo-arm", default=None, choices=sorted(NEMO_ARMS), help="one arm of --nemo in this process (what --nemo starts)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.streams and a.nemo_arm:
        return nemo_arm(a.nemo_arm, a.streams, passes=a.passes)
    if a.streams and a.nemo:
        return nemo_bench(a.streams, a.out, a.parent_library, repeats=a.repeats, passes=a.passes, chunks=a.chunks)
    if a.streams and a.out_rate:
        return output_bench(a.streams, a.out, a.rate or FS, a.out_rate, a.out_pcm16, pinned=a.pinned, passes=a.passes)
    if a.streams:
        return group_bench(a.streams, a.out, handoff=a.handoff, only_grouped=a.only_grouped, pcm16=a.pcm16, pinned=a.pinned, rate=a.rate,
                           preview=a.preview, passes=a.passes, window=a.window and a.handoff, history=a.history and a.handoff)
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
