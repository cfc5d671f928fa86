"""Separate a meeting while it happens: a synthetic 7-channel meeting is fed to a CssStream in 0.5 s chunks, as a live
source would deliver it; every push returns the samples of the three separated streams that have become final (equal, bit
for bit, to the offline result on the whole meeting).  Prints the lag and the time of each push.

With --rooms N, N synthetic meetings (different seeds) arrive tick by tick and are pushed through one CssStreamGroup: the
segments the rooms complete in a tick share the mask estimator's batches (css_stream_push_many).

With --logmel every stream has the hand-off to the ASR front end on: each tick also returns, per room and speaker, the raw
Whisper log-mel frames and the sample ranges of the audio the activity gate kept (CssStream(handoff=...)); a Whisper host
collects 3 000 frames per window and normalises each window with whisper_normalize.

With --pcm16 the source delivers 16-bit PCM, as a capture device does: the int16 chunks go to push_pcm16 as they are (2 bytes
per sample over PCIe, scaled and de-interleaved on the device); the result is that of pushing chunk.astype(float32) / 32768.

With --rate HZ the source delivers 16-bit PCM at HZ (48000, 44100, 32000, 8000 ...): the stream is opened with input_rate=HZ,
the int16 chunks cross PCIe as they were captured and the ingest kernel resamples them to the model's 16 kHz
(scipy.signal.resample_poly's default filter); what comes back stays at 16 kHz.

With --preview every tick also asks for the unfinished tail (CssStream.preview / CssStreamGroup.preview): the provisional
samples between the final ones and the present -- css_run of what was pushed so far -- while the stream stays as it was.  Each
tick prints how far the final and the provisional output reach behind the input; a caption host shows the provisional part
at once and replaces it as it becomes final.  With --preview --logmel the preview also hands off (preview(handoff=True)): the
provisional log-mel frames and kept seconds up to the present are printed next to the final ones; the host places them behind
frame preview_handoff.first_frame[k] of speaker k's frames so far and normalises with preview_handoff.raw_max[k].

With --window (implies --logmel) every stream also keeps its last 3 000 raw frames on the device
(CssStream(window_history=3000)) and every tick ends with ONE call that writes a Whisper encoder input per room and speaker --
the last frames, normalised over the window, padded to 3 000 columns, float16 -- into a torch tensor on the GPU
(CssStream.window / CssStreamGroup.windows): what a PyTorch-ROCm Whisper encoder takes, without the frames crossing PCIe again.

With --present (implies --window) the windows reach the present: ONE call per tick previews every room and writes, per room and
speaker, the last frames of the history followed by the preview's provisional frames, normalised over the whole span
(CssStream.present_window / CssStreamGroup.present_windows) -- an encoder input that ends at the microphone instead of up to
3.6 s behind it, without the provisional frames going through the host.

With --out-rate HZ [--out-pcm16] the final samples come back at the playback rate HZ, as float32 or (--out-pcm16) 16-bit PCM,
resampled, scaled and rounded on the device (CssStream(output=dict(rate=HZ, dtype="int16"))): what a conference bridge that
takes 48 kHz PCM16 and plays 48 kHz PCM16 needs, with nothing crossing PCIe at the model rate.  The previews stay float32 at
the model rate.

With --nemo every stream has the NeMo hand-off on instead (CssStream(nemo=...), include/css_mi355_stream_nemo.h): each tick also
returns, per room and speaker, the raw NeMo frames ln(mel + 2^-24) that became complete and the kept ranges -- what a cache-aware
streaming FastConformer, a streaming diarizer or a frame-level VAD on the same GPU takes (they normalise per short window
themselves, or not at all).  A stream has one format: --nemo does not go with --logmel, --window or --present; a plain --preview does.

With --nemo --chunks the streams also keep their last 1024 NeMo frames on the device (CssStream(nemo_history=1024),
include/css_mi355_nemo_chunk.h) and after every tick ONE call writes, per room and speaker, two chunks into torch tensors on the
GPU: the raw [80, 70 + 14] frames a cache-aware streaming FastConformer step takes (pre-encode cache + chunk) and a 4 s buffer
normalised per feature over the buffer, float16 -- what FrameBatchASR, a streaming diarizer or a frame-level VAD takes -- without
the frames crossing PCIe again (CssStream.nemo_chunk / CssStreamGroup.nemo_chunks).

    python examples/live_stream.py [--seconds 30] [--rooms N] [--logmel | --nemo [--chunks]] [--pcm16] [--rate HZ] [--preview]
                                   [--window] [--present] [--out-rate HZ] [--out-pcm16]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import notsofar1_challenge_amd.css as CSS          # noqa: E402
import notsofar1_challenge_amd.separator as SEP    # noqa: E402
import notsofar1_challenge_amd.stream as STR       # noqa: E402
import notsofar1_challenge_amd.synth as SYN        # noqa: E402
import notsofar1_challenge_amd.weights as W        # noqa: E402


HANDOFF = dict(n_mels=80, pad_frames=8, drop_silence=True)
NEMO = dict(n_mels=80, pad_frames=8, drop_silence=True, preemphasis=0.97)


def print_handoff(streams, fs):
    """per room and speaker: log-mel frames and kept seconds of this tick"""
    for r, s in enumerate(streams):
        h = s.handoff
        per = [f"{m.shape[1]:4d} fr {float((g[:, 1] - g[:, 0]).sum()) / fs:5.2f} s" for m, g in zip(h.mel, h.ranges)]
        print(f"    room {r}: " + " | ".join(per))


def print_nemo(streams, fs):
    """per room and speaker: NeMo frames of this tick (from which frame of the concatenation on) and kept seconds"""
    for r, s in enumerate(streams):
        h = s.nemo
        per = [f"{m.shape[1]:4d} fr from {int(f0):5d} {float((g[:, 1] - g[:, 0]).sum()) / fs:5.2f} s" for m, g, f0 in zip(h.mel, h.ranges, h.first_frame)]
        print(f"    room {r}: " + " | ".join(per))


def print_preview_handoff(streams, fs):
    """per room and speaker: provisional log-mel frames (from which frame of the concatenation on) and kept seconds"""
    for r, s in enumerate(streams):
        h = s.preview_handoff
        if h is None:
            continue
        per = [f"{m.shape[1]:4d} fr from {int(j):5d} {float((g[:, 1] - g[:, 0]).sum()) / fs:5.2f} s" for m, g, j in zip(h.mel, h.ranges, h.first_frame)]
        print(f"    room {r} provisional: " + " | ".join(per))


def capture(mix):
    """what a 16-bit capture device would have delivered: [n, 7] int16, interleaved"""
    return np.clip(np.rint(mix.astype(np.float64) * 0.2 * 32768.0), -32768, 32767).astype(np.int16)


def capture_at(mix, fs, rate):
    """the meeting as a 16-bit capture device running at `rate` would have delivered it (linear interpolation of the synthetic
    16 kHz samples: a stand-in for a real device, not a resampler)"""
    t = np.arange(int(round(mix.shape[0] * rate / fs))) * (float(fs) / rate)
    at = np.arange(mix.shape[0])
    return capture(np.stack([np.interp(t, at, mix[:, c]) for c in range(mix.shape[1])], axis=1))


def behind(inf, first, count, fs):
    """how far the final and the provisional output end behind the input's last sample, in seconds (count None: no preview yet)"""
    final = f"final {(inf.n_pushed - inf.n_emitted) / fs:4.2f} s behind"
    if count is None:
        return final + ", no preview yet (css_run refuses a recording of at most one segment)"
    return final + f", provisional {max(inf.n_pushed - (first + count), 0) / fs:4.2f} s behind ({count / fs:4.2f} s of preview)"


def encoder_windows(group, streams, batch):
    """one css_stream_windows for every (room, speaker) that holds a frame -> the float16 batch [B, 80, 3000] on the device"""
    reqs = []
    for s in streams:
        first, end = s.window_range()
        reqs += [(s, k) for k in range(s.num_spks) if end[k] > first[k]]
    if not reqs:
        print("    no encoder windows yet")
        return None
    t = time.perf_counter()
    out = group.windows(reqs, out=batch[:len(reqs)])
    ms = (time.perf_counter() - t) * 1e3
    print(f"    {len(reqs)} encoder windows {tuple(out.shape)} {out.dtype} on {out.device} in {ms:5.2f} ms, "
          f"{group.window_launches} launch(es)")
    return out


def present_windows(group, streams, batch):
    """one css_stream_present_windows for every (room, speaker): the preview of all rooms and the float16 batch [B, 80, 3000] that
    ends at the present, on the device; rows of rooms without a preview or a frame yet stay unwritten (n_used 0)"""
    reqs = [(s, k) for s in streams for k in range(s.num_spks)]
    t = time.perf_counter()
    out, spans, _ = group.present_windows(reqs, out=batch[:len(reqs)])
    ms = (time.perf_counter() - t) * 1e3
    live = spans[:, 1] > 0
    print(f"    {int(live.sum())} of {len(reqs)} encoder windows up to the present in {ms:5.2f} ms, {group.window_launches} launch(es); "
          f"frames per window {spans[live, 1].tolist()}, of them provisional {spans[live, 2].tolist()}")
    return out, live


def nemo_chunks(group, streams, step, buffered):
    """one css_stream_nemo_chunks per kind for every (room, speaker) that holds enough frames: the raw step input [B, 80, 84] of a
    cache-aware encoder into `step`, and the last 4 s normalised per feature over the buffer, float16 [B, 80, 400], into `buffered`"""
    for what, width, normalize, batch in (("raw step inputs", step.shape[2], None, step), ("per-feature buffers", buffered.shape[2], "per_feature", buffered)):
        reqs = [(s, k, None, width) for s in streams for k in range(s.num_spks) if s.nemo_history_range()[1][k] >= width]
        if not reqs:
            print(f"    no {what} yet")
            continue
        t = time.perf_counter()
        out = group.nemo_chunks(reqs, width, normalize, str(batch.dtype).split(".")[1], out=batch[:len(reqs)])
        ms = (time.perf_counter() - t) * 1e3
        print(f"    {len(reqs)} {what} {tuple(out.shape)} {out.dtype} on {out.device} in {ms:5.2f} ms, {group.window_launches} launch(es)")


def chunk_batches(n, n_mels):
    import torch
    return (torch.empty((n, n_mels, 70 + 14), dtype=torch.float32, device="cuda"), torch.empty((n, n_mels, 400), dtype=torch.float16, device="cuda"))


def rooms(sep, n_rooms, seconds, fs, chunk, logmel=False, pcm16=False, rate=None, preview=False, window=False, present=False, output=None,
          nemo=False, chunks=False):
    mixes = [SYN.synth_meeting(seconds, 7, seed=1 + r)[0] for r in range(n_rooms)]
    if rate:
        mixes = [capture_at(m, fs, rate) for m in mixes]
        chunk = chunk * rate // fs
    elif pcm16:
        mixes = [capture(m) for m in mixes]
    streams = [STR.CssStream(sep, CSS.CssCfg(), fs=fs, num_channels=7, handoff=HANDOFF if logmel else None, input_rate=rate,
                             window_history=3000 if window else None, output=output, nemo=NEMO if nemo else None,
                             nemo_history=1024 if chunks else None) for _ in mixes]
    group = STR.CssStreamGroup(streams)
    if chunks:
        step, buffered = chunk_batches(n_rooms * sep.desc.num_spks, NEMO["n_mels"])
    if window:
        import torch
        batch = torch.empty((n_rooms * sep.desc.num_spks, HANDOFF["n_mels"], 3000), dtype=torch.float16, device="cuda")
    outs = [[[] for _ in range(sep.desc.num_spks)] for _ in mixes]
    print(f"{n_rooms} rooms, lag bound {streams[0].latency_samples / fs:.2f} s")
    for i in range(0, mixes[0].shape[0], chunk):
        t = time.perf_counter()
        res = (group.push_pcm16 if pcm16 else group.push)([m[i:i + chunk] for m in mixes])
        ms = (time.perf_counter() - t) * 1e3
        for room, got in zip(outs, res):
            for k, o in enumerate(got):
                room[k].append(o)
        inf = streams[0].info()
        print(f"t={inf.n_pushed / fs:6.1f} s  final={inf.n_emitted / fs:6.1f} s  tick {ms:6.2f} ms  "
              f"estimator batches {group.stats.estimator_batches} ({group.stats.estimator_segments} segments)")
        if logmel:
            print_handoff(streams, fs)
        if nemo:
            print_nemo(streams, fs)   # -> the streaming encoder's next chunk: torch.from_numpy(s.nemo.mel[k])[None]
        if chunks:
            nemo_chunks(group, streams, step, buffered)   # -> encoder.cache_aware_stream_step(step[:B]) / asr(buffered[:B]) on the same GPU
        if preview:
            t = time.perf_counter()
            pv = group.preview(handoff=logmel)
            ms = (time.perf_counter() - t) * 1e3
            print(f"    preview {ms:6.2f} ms, one batch of {group.stats.estimator_segments} segments; room 0: "
                  + behind(inf, streams[0].preview_first_sample, None if pv[0] is None else pv[0][0].shape[0], fs))
            if logmel:
                print_preview_handoff(streams, fs)
        if window:
            encoder_windows(group, streams, batch)   # -> whisper_encoder(batch[:B]) on the same GPU
        if present:
            present_windows(group, streams, batch)   # -> whisper_encoder(batch[live]): captions up to the present
    for s, room in zip(streams, outs):
        for k, o in enumerate(s.finish()):
            room[k].append(o)
        s.close()
    print("separated:", [[np.concatenate(x).shape[0] / (output["rate"] if output else fs) for x in room] for room in outs], "s")
    if output:
        print("samples the PCM16 clamp changed, per room:", [s_.output_clipped.tolist() for s_ in streams])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--rooms", type=int, default=1, help="meetings fed tick by tick through one CssStreamGroup")
    ap.add_argument("--logmel", action="store_true", help="also return Whisper log-mel frames and kept ranges with every tick")
    ap.add_argument("--nemo", action="store_true", help="also return raw NeMo log-mel frames and kept ranges with every tick (not with --logmel)")
    ap.add_argument("--chunks", action="store_true", help="with --nemo: after each tick, a NeMo consumer's chunks per room and speaker in torch tensors on the GPU")
    ap.add_argument("--pcm16", action="store_true", help="the source delivers int16 samples: push_pcm16 instead of push")
    ap.add_argument("--preview", action="store_true", help="after each tick's push, also fetch the provisional tail (preview)")
    ap.add_argument("--rate", type=int, default=0, help="the source delivers int16 samples at this rate: CssStream(input_rate=HZ)")
    ap.add_argument("--window", action="store_true", help="after each tick, Whisper encoder windows per room and speaker in a torch tensor on the GPU")
    ap.add_argument("--present", action="store_true", help="after each tick, encoder windows that end at the present: the history and a preview's frames in one call")
    ap.add_argument("--out-rate", type=int, default=0, help="the final samples come back at this rate, converted on the device: CssStream(output=dict(rate=HZ))")
    ap.add_argument("--out-pcm16", action="store_true", help="... as int16 (gain 1, no peak normalisation); alone: int16 at the model rate")
    a = ap.parse_args()
    fs = 16000
    a.window = a.window or a.present
    a.logmel = a.logmel or a.window
    if a.nemo and a.logmel:
        ap.error("--nemo is a hand-off format of its own: not with --logmel, --window or --present")
    if a.chunks and not a.nemo:
        ap.error("--chunks are a NeMo consumer's: with --nemo")
    a.pcm16 = a.pcm16 or bool(a.rate)
    output = dict(rate=a.out_rate or fs, dtype="int16" if a.out_pcm16 else "float32") if a.out_rate or a.out_pcm16 else None
    desc = W.ModelDesc.mc_v1()
    sep = SEP.HipSeparator(W.apply_golden_recipe(W.portable_state_dict(desc, 0)), None, device=0)
    if a.rooms > 1:
        rooms(sep, a.rooms, a.seconds, fs, fs // 2, a.logmel, a.pcm16, a.rate or None, a.preview, a.window, a.present, output, a.nemo, a.chunks)
        sep.close()
        return
    mix = SYN.synth_meeting(a.seconds, 7, seed=1)[0]
    if a.rate:
        mix = capture_at(mix, fs, a.rate)
    elif a.pcm16:
        mix = capture(mix)
    chunk = (a.rate or fs) // 2
    streams = [[] for _ in range(desc.num_spks)]
    mels = [[] for _ in range(desc.num_spks)]
    with STR.CssStream(sep, CSS.CssCfg(), fs=fs, num_channels=7, handoff=HANDOFF if a.logmel else None, input_rate=a.rate or None,
                       window_history=3000 if a.window else None, output=output, nemo=NEMO if a.nemo else None,
                       nemo_history=1024 if a.chunks else None) as s:
        if a.chunks:
            step, buffered = chunk_batches(desc.num_spks, NEMO["n_mels"])
        if a.window:
            import torch
            batch = torch.empty((desc.num_spks, HANDOFF["n_mels"], 3000), dtype=torch.float16, device="cuda")
        print(f"lag bound {s.latency_samples / fs:.2f} s" + (f" + {s.resampler_lag_samples} input samples of the resampler" if s.rate else ""))
        for i in range(0, mix.shape[0], chunk):
            t = time.perf_counter()
            out = (s.push_pcm16 if a.pcm16 else s.push)(mix[i:i + chunk])
            ms = (time.perf_counter() - t) * 1e3
            for k, o in enumerate(out):
                streams[k].append(o)
            inf = s.info()
            print(f"t={inf.n_pushed / fs:6.1f} s  final={inf.n_emitted / fs:6.1f} s  lag={(inf.n_pushed - inf.n_emitted) / fs:4.2f} s  "
                  f"push {ms:6.2f} ms" + (f"  {out[0].shape[0]} {out[0].dtype} samples at {output['rate']} Hz" if output else ""))
            if a.logmel:
                print_handoff([s], fs)
                for k, m in enumerate(s.handoff.mel):
                    mels[k].append(m)
            if a.nemo:
                print_nemo([s], fs)
                for k, m in enumerate(s.nemo.mel):
                    mels[k].append(m)
            if a.chunks:
                nemo_chunks(STR.CssStreamGroup([s]), [s], step, buffered)
            if a.preview:
                try:
                    count = s.preview(handoff=a.logmel)[0].shape[0]
                except AssertionError:   # css_run's own refusal of a recording of at most one segment (css.py:297)
                    count = None
                print("    " + behind(inf, s.preview_first_sample, count, fs))
                if a.logmel and count is not None:
                    print_preview_handoff([s], fs)
            if a.window:
                encoder_windows(STR.CssStreamGroup([s]), [s], batch)
            if a.present:
                present_windows(STR.CssStreamGroup([s]), [s], batch)
        for k, o in enumerate(s.finish()):
            streams[k].append(o)
        if a.nemo:
            for k, m in enumerate(s.nemo.mel):
                mels[k].append(m)
            for k in range(desc.num_spks):
                print(f"speaker {k}: {np.concatenate(mels[k], axis=1).shape[1]} NeMo frames in all")
        if a.logmel:
            for k, m in enumerate(s.handoff.mel):
                mels[k].append(m)
            # a Whisper host: windows of 3 000 frames, each normalised with its own maximum
            for k in range(desc.num_spks):
                raw = np.concatenate(mels[k], axis=1)
                windows = [STR.whisper_normalize(raw[:, i:i + 3000]) for i in range(0, raw.shape[1], 3000)]
                print(f"speaker {k}: {raw.shape[1]} log-mel frames in {len(windows)} Whisper window(s)")
    wavs = [np.concatenate(x) for x in streams]
    print("separated:", [w.shape[0] / (output["rate"] if output else fs) for w in wavs], "s")
    sep.close()


if __name__ == "__main__":
    main()
