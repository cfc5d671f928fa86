"""Exact models of the kernels every live stream runs on every push -- csrc/stream.hip (activity, gate + overlap-add, mask scatter,
PCM16 ingest) and the streamed part of csrc/handoff.hip (append, mel) -- the case lists of tests/test_hip_stream_kernels.py and the
named mistakes as `mut` switches of the models (DESIGN.md 7b "The stream kernels, launch form by launch form").  No GPU, no
library: tests/test_stream_reference.py checks this file on the CPU.

Every model but the mel values is exact: these kernels round nowhere, or in the stated order of csrc/stitch_common.hpp, which
backend_reference restates (products, sums from 0 in ascending segment order, one division; the frequency mean as float64 sums of
16 groups).  The models here generalise those to a WINDOW of segment slots:
  slot j is segment seg_base + j and starts at local frame j hop; local frame t is frame t + frame_base of the recording;
  first / last weights go by the global index, and no segment is the last one while num_segments_global is OPEN;
  dilation sees zeros and erosion sees ones outside the recording, [-frame_base, T_long_global - frame_base) in local frames;
  a row of Y is [Re F | Im F | zeros up to KIp]; the gate byte of local frame t lands at ring column (t + frame_base) & (gate_ld - 1).
The append model is stated on the concatenation itself: block q of 256 samples is kept iff a gated-final active frame t has
t - pad <= q <= t + pad + 1 (handoff_reference.kept_ranges in block form), the kept samples of [D0, D1) go behind the A0 already
there, J frames are complete (n // 160 when closing, (n - 200) // 160 + 1 from n >= 201 on while open) and operand column x of a
speaker is sample 160 J0 + x of the reflect-padded concatenation (handoff_reference.operand, with the gather kernel's clamp below
201 samples).  tests/test_stream_reference.py proves that any cutting into rounds composes to handoff_reference's whole-recording
concatenation, frame count and operand, and that any sequence of windows and ranges composes to backend_reference's results.

Which operand columns are DEFINED values: the columns a frame of the round reads, [0, 160 (n_new - 1) + 400) for n_new > 0 (the
product reads 416 columns per row; columns 400 .. 415 meet zeros of the matrix).  The columns behind them, up to 160 rows, are
"finite, not read by a completed frame" (zeros, or before closing samples already known); append_round returns both and
`defined`, the count of the former.

`mut` names one deliberate mistake (TAIL_MISTAKES, APPEND_MISTAKES, MEL_MISTAKES, INGEST_MISTAKES); None is the definition."""
import numpy as np

import backend_reference as B
import handoff_reference as H
from frontend_reference import CANARY, U, bits, canary  # noqa: F401  (shared with the other kernel tests)

f32 = np.float32
OPEN = 2 ** 63 - 1                      # INT64_MAX: the stream is open
CANARY_BYTE = B.CANARY_BYTE
CANARY16 = np.int16(0x5A5A)
CANARY32 = np.int32(0x5A5A5A5A)
STATE = np.dtype([("A", "<i8"), ("J", "<i8"), ("gmax", "<i4"), ("pad", "<i4")])
GMAX_NONE = np.int32(-2139095041)       # 0x807fffff: -inf in the order-preserving integer form (HANDOFF_GMAX_NONE)
TAIL_LD = 512                           # HANDOFF_TAIL_LD
OLA_T = 16                              # frames per block of the gate kernel

TAIL_MISTAKES = ("local_weights", "last_while_open", "erode_zeros_outside", "dilate_ones_outside", "halo_wrong_row", "ring_no_base",
                 "pad_unwritten")
APPEND_MISTAKES = ("keep_lo_off", "keep_hi_off", "keep_past_tg1", "second_pass_restarts", "last_block_uncut", "J_open_on_closing",
                   "J_closing_on_open", "right_edge_repeat", "tail_from_J0", "carry_from_out_base")
# The reflection without the clamp at A1 < 201 is a mistake of another kind: an index goes below sample 0 only for A1 < 101, where no
# frame is complete, so no DEFINED column can differ (tests/test_stream_reference.py proves it for every A1); what it would do is
# read below the speaker's row, which the GPU test meets with finiteness: the floats there are NaN.
APPEND_MISTAKES_UNREAD = ("no_clamp",)
MEL_MISTAKES = ("slot_without_count", "first_hist_kept", "signed_bits_max")
INGEST_MISTAKES = ("scale_32767", "tail_dropped")


def canary8(n):
    return np.full(int(n), CANARY_BYTE, np.uint8)


# ---- the stitching tail over a window -----------------------------------------------------------------------------------------

def _covering(t, T, hop, num_slots):
    lo = t - T + 1
    s0 = 0 if lo <= 0 else -(-lo // hop)
    return range(s0, min(t // hop, num_slots - 1) + 1)


def _frame(rows, w, windows, perms, t, mut):
    """backend_reference._ola_frame over the window w (a dict with S, T, hop, num_slots, seg_base, num_segments_global)"""
    segs = list(_covering(t, w["T"], w["hop"], w["num_slots"]))
    nsg = w["num_segments_global"]
    if mut == "last_while_open" and nsg == OPEN:
        nsg = w["seg_base"] + w["num_slots"]

    def weight(seg):
        return B._weights(windows, seg if mut == "local_weights" else w["seg_base"] + seg, nsg)[t - seg * w["hop"]]

    ws = f32(0)
    for seg in segs:
        ws = f32(ws + weight(seg))
    out = []
    for s in range(w["S"]):
        v = None
        for seg in segs:
            term = weight(seg) * rows(seg, perms[seg][s], t - seg * w["hop"])
            v = (np.zeros_like(term) + term) if v is None else v + term
        out.append(None if v is None else v / ws)
    return out, bool(segs)


def activity(w, masks, windows, perms, t_lo, t_hi, act_b, mut=None):
    """launch_stream_activity_multi of one job on the allocation act_b [S][ld_frames] (a copy is returned)"""
    F, T = w["F"], w["T"]
    m = np.asarray(masks, np.float32).reshape(-1, F, w["mask_ld"])
    act_b = act_b.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(t_lo, t_hi):
            vals, any_ = _frame(lambda seg, k, tl: m[k, :, seg * T + tl], w, windows, perms, t, mut)
            for s in range(w["S"]):
                if not any_:
                    act_b[s, t] = 0          # (0 / 0: a NaN mean is not >= th)
                    continue
                v = vals[s].astype(np.float32)
                tot = 0.0
                for g in range(16):
                    part = 0.0
                    for x in v[g::16]:
                        part += float(x)
                    tot += part
                act_b[s, t] = f32(tot / float(F)) >= f32(w["activity_th"])
    return act_b


def morph_reads(w, t_lo, t_hi, blocks=False):
    """the local frames of act_b whose value can reach an output of [t_lo, t_hi) (blocks: every frame the kernel looks at: its
    blocks of 16 dilate whole; those at or above ld_frames it reads as 0) -- [lo, hi)"""
    halo = w["erosion"] + w["dilation"]
    hi = t_lo + -(-(t_hi - t_lo) // OLA_T) * OLA_T if blocks else t_hi
    g_end = w["T_long_global"] - w["frame_base"]
    return max(t_lo - halo, -w["frame_base"]), min(hi + halo, g_end)


def gate_bytes(w, act_b, t_lo, t_hi, mut=None):
    """[S][t_hi - t_lo]: erode(dilate(act_b)) at the local frames [t_lo, t_hi)"""
    S, d, e, fb = w["S"], w["dilation"], w["erosion"], w["frame_base"]
    g_end = w["T_long_global"] - fb
    out = np.zeros((S, t_hi - t_lo), np.uint8)
    outside = lambda u: u + fb < 0 or u >= g_end
    for s in range(S):
        def at(x):
            if outside(x):
                return 1 if mut == "dilate_ones_outside" else 0
            return act_b[(s + 1) % S if mut == "halo_wrong_row" and x < t_lo else s, x] != 0
        for t in range(t_lo, t_hi):
            keep = 1
            for u_ in range(t - e, t + e + 1):
                if outside(u_):
                    x = 0 if mut == "erode_zeros_outside" else 1
                else:
                    x = int(any(at(x_) for x_ in range(u_ - d, u_ + d + 1)))
                keep &= x
            out[s, t - t_lo] = keep
    return out


def gate_ola(w, sep, windows, perms, act_b, t_lo, t_hi, Y, ring, mut=None):
    """launch_stream_gate_ola_multi of one job on the allocations Y [S][ld_frames][KIp] and ring [S][gate_ld] or None (copies are
    returned)"""
    F, KIp, fb = w["F"], w["KIp"], w["frame_base"]
    Y = Y.copy()
    ring = None if ring is None else ring.copy()
    keep = gate_bytes(w, act_b, t_lo, t_hi, mut)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(t_lo, t_hi):
            vals, any_ = _frame(lambda seg, k, tl: sep[seg, k, :, tl, :], w, windows, perms, t, mut)
            for s in range(w["S"]):
                row = Y[s, t].copy() if mut == "pad_unwritten" else np.zeros(KIp, np.float32)
                row[:2 * F] = 0
                if any_:
                    v = vals[s].astype(np.float32) * (f32(1) if keep[s, t - t_lo] else f32(0))
                    row[:F], row[F:2 * F] = v[:, 0], v[:, 1]
                Y[s, t] = row
                if ring is not None:
                    ring[s, (t + (0 if mut == "ring_no_base" else fb)) & (ring.shape[1] - 1)] = keep[s, t - t_lo]
    return Y, ring


def dilate_erode(row, T_long, d, e):
    """the whole recording's gate: zeros outside for the dilation, ones for the erosion (css.py:303-312)"""
    p = np.pad(row.astype(np.uint8), d)
    dil = np.lib.stride_tricks.sliding_window_view(p, 2 * d + 1).max(1) if T_long else p
    p = np.pad(dil, e, constant_values=1)
    return np.lib.stride_tricks.sliding_window_view(p, 2 * e + 1).min(1) if T_long else p


# ---- tail cases ---------------------------------------------------------------------------------------------------------------
# A case is a RECORDING (N segments of T frames at hop, S, F, KIp, a threshold, a morphology, a gate kind) and a list of windows,
# each (seg_base, num_slots, closed, ranges); ld_frames holds the frames the range's gate is taken from and not a frame more, so the
# last block's idle lanes look past the row's end (the kernel reads 0 there).

GATE_KINDS = ("random", "all_on", "all_off", "edges", "range_edges")


def tail_recording(c):
    """the whole recording's inputs, computed once per case: masks [(S + 1) F][N T], sep [N][S][F][T][2], windows [3][T], perms
    [N][S], gate_in [S][TL] (the activity bytes the gate launches are given)"""
    if "_rec" in c:
        return c["_rec"]
    S, F, T, N = c["S"], c["F"], c["T"], c["N"]
    rng = np.random.default_rng(c["seed"])
    masks = rng.uniform(0, 1, ((S + 1) * F, N * T)).astype(np.float32)
    if c.get("threshold_rows"):
        # rows whose frequency mean is exactly th, and its two float32 neighbours, in every frame of speaker 0 / 1 / 2: all F bins
        # hold the same value v; with every window weight 0.5 and at most two contributors w v, w v + w v and the quotient by w
        # or 2 w are exact, and the float64 sum of F equal float32 values and its quotient by F are exact too: the mean IS v
        th = f32(c["th"])
        for k, v in enumerate((th, np.nextafter(th, f32(0)), np.nextafter(th, f32(1)))[:S]):
            masks[k * F:(k + 1) * F, :] = v
    sep = rng.standard_normal((N, S, F, T, 2)).astype(np.float32)
    if c.get("threshold_rows"):
        assert -(-T // c["hop"]) <= 2
        windows = np.full((3, T), 0.5, np.float32)
    else:
        windows = B.ola_windows("random", T, c["seed"] + 1, None)
    perms = B.ola_perms("identity" if c.get("threshold_rows") else "random", S, N, c["seed"] + 2)
    TL = c["TL"]
    kind = c["gate"]
    if kind == "random":
        g = B.gates(S, TL, c["seed"] + 3)
    elif kind == "all_on":
        g = np.ones((S, TL), np.uint8)
    elif kind == "all_off":
        g = np.zeros((S, TL), np.uint8)
    elif kind == "edges":
        g = np.zeros((S, TL), np.uint8)
        g[:, 0] = 1
        g[-1, TL - 1] = 1
    else:   # single frames at both edges of every range of every window
        g = np.zeros((S, TL), np.uint8)
        for wd in c["windows"]:
            fb = wd["seg_base"] * c["hop"]
            for lo, hi in wd["ranges"]:
                if hi > lo:
                    g[0, fb + lo] = 1
                    g[-1, fb + hi - 1] = 1
    c["_rec"] = dict(masks=masks, sep=sep, windows=windows, perms=perms, gate_in=g)
    return c["_rec"]


def window_of(c, wd):
    """the StreamStitchArgs scalars of a window of a case"""
    T, hop = c["T"], c["hop"]
    b, n, closed = wd["seg_base"], wd["num_slots"], wd["closed"]
    return dict(S=c["S"], F=c["F"], T=T, hop=hop, KIp=c["KIp"], dilation=c["dilation"], erosion=c["erosion"], activity_th=c["th"],
                num_slots=n, seg_base=b, frame_base=b * hop, num_segments_global=c["N"] if closed else OPEN,
                T_long_global=c["TL"] if closed else OPEN, mask_ld=n * T + wd.get("mask_pad", 0), ld_frames=wd["ld_frames"],
                gate_ld=c["gate_ld"])


def window_inputs(c, wd):
    """the window's arrays cut from the recording: masks [(S + 1) F][mask_ld], sep, perms of its slots, windows, and act_b
    [S][ld_frames]: the recording's gate_in at the frames the window holds, CANARY_BYTE elsewhere"""
    r = tail_recording(c)
    w = window_of(c, wd)
    b, n, T = wd["seg_base"], wd["num_slots"], c["T"]
    masks = np.full(((c["S"] + 1) * c["F"], w["mask_ld"]), np.nan, np.float32)
    masks[:, :n * T] = r["masks"][:, b * T:(b + n) * T]
    act = canary8(c["S"] * w["ld_frames"]).reshape(c["S"], -1)
    fb = w["frame_base"]
    hi = min(w["ld_frames"], c["TL"] - fb)
    act[:, :hi] = r["gate_in"][:, fb:fb + hi]
    return w, dict(masks=masks, sep=r["sep"][b:b + n], perms=r["perms"][b:b + n], w_first=r["windows"][0], w_mid=r["windows"][1],
                   w_last=r["windows"][2], act_b=act)


def final_frames(c, wd):
    """the local frames [lo, hi) of a window that all their covering segments lie in (what a path may ask of it)"""
    T, hop, b, n = c["T"], c["hop"], wd["seg_base"], wd["num_slots"]
    lo = 0 if b == 0 else T - hop
    hi = c["TL"] - b * hop if wd["closed"] else n * hop
    return lo, hi


def _tail_case(i, T, hop, N, S, F, extra, dil, ero, gate, windows, **kw):
    KIp = 2 * F if extra == 0 else (2 * F + 31) // 32 * 32 + (32 if extra == 2 else 0)
    cov = B.coverage(N, T, hop)
    c = dict(name=f"T{T}_hop{hop}_N{N}_S{S}_F{F}_d{dil}_e{ero}_{gate}_{i}", T=T, hop=hop, N=N, S=S, F=F, KIp=KIp, dilation=dil, erosion=ero,
             gate=gate, TL=cov - kw.pop("cut", 0), th=kw.pop("th", 0.5), gate_ld=kw.pop("gate_ld", 64), seed=900 + i, windows=[], **kw)
    for b, n, closed, ranges in windows:
        wd = dict(seg_base=b, num_slots=n, closed=closed, ranges=ranges, mask_pad=(0, 3)[(i + b) % 2])
        reach = max([hi - 1 + dil + ero for lo, hi in ranges if hi > lo] + [0])
        top = max(hi for _, hi in ranges)
        g_end = c["TL"] - b * hop if closed else OPEN
        wd["ld_frames"] = max(min(reach, g_end - 1) + 1, top, 1, c.get("ld_min", 0))
        flo, fhi = final_frames(c, wd)
        for lo, hi in ranges:
            assert flo <= lo <= hi <= fhi, (c["name"], wd, (flo, fhi))
            assert b == 0 or lo >= dil + ero or hi == lo, (c["name"], wd)
        c["windows"].append(wd)
    return c


def tail_cases():
    """(T, hop) x F x S x KIp x windows x ranges x morphology x gates, rotated; every line says what it is there for"""
    out = []
    add = lambda *a, **k: out.append(_tail_case(len(out), *a, **k))
    # one contributor; base 0 and open: lengths 0, 1, 15, 16, 17, 33, t_lo not a multiple of 16
    add(8, 8, 9, 1, 5, 0, 0, 0, "random", [(0, 9, False, [(0, 0), (0, 1), (1, 16), (16, 32), (3, 20), (5, 38), (38, 72)])])
    # two contributors: base > 0 and open (local / global weights, w_last while open), then the last segment inside the window
    add(8, 4, 12, 3, 16, 1, 3, 1, "random", [(0, 6, False, [(0, 17), (17, 24)]), (3, 5, False, [(4, 5), (5, 20)]),
                                             (6, 6, True, [(4, 21), (21, 28)])])
    # three contributors; closing with T_long_global inside a block of 16 (cut 3)
    add(8, 3, 10, 4, 17, 2, 5, 0, "all_off", [(0, 10, True, [(0, 16), (16, 33)]), (4, 6, True, [(5, 20)])], cut=2)
    add(8, 3, 10, 3, 5, 0, 0, 5, "all_on", [(0, 10, True, [(0, 33), (33, 35)]), (5, 5, True, [(5, 20)])])
    # sixteen contributors
    add(16, 1, 30, 4, 5, 1, 3, 1, "edges", [(0, 30, False, [(0, 30)]), (7, 20, False, [(15, 16), (16, 20)]), (12, 18, True, [(15, 33)])])
    # the default segmentation at F 257 (and a small F beside it)
    add(186, 179, 2, 3, 257, 1, 3, 1, "random", [(0, 2, False, [(170, 187)]), (1, 1, True, [(7, 24)])])
    add(186, 179, 3, 3, 17, 2, 5, 0, "range_edges", [(0, 2, False, [(0, 15), (15, 31), (175, 208)]), (1, 2, True, [(7, 40), (345, 360)])], cut=5)
    # the staging loop over more than 256 bytes: erosion 130 (OLA_T + 2 * 130 = 276)
    add(8, 4, 100, 3, 5, 0, 2, 130, "random", [(0, 80, False, [(0, 17), (140, 173)]), (20, 50, False, [(132, 149)]),
                                               (60, 40, True, [(133, 164)])])
    add(8, 4, 80, 1, 16, 1, 2, 130, "all_on", [(0, 80, True, [(0, 33), (300, 324)])])
    # erosion at the recording's first frame and dilation at its last (zeros / ones outside), single frames at the range edges
    add(8, 4, 12, 3, 16, 0, 0, 5, "range_edges", [(0, 12, True, [(0, 16), (35, 52)]), (5, 7, True, [(5, 21), (31, 32)])])
    add(8, 8, 6, 4, 5, 2, 5, 0, "edges", [(0, 6, True, [(0, 48)]), (2, 4, True, [(5, 32)])])
    add(16, 1, 40, 3, 17, 1, 0, 0, "random", [(20, 20, False, [(15, 20)]), (20, 20, True, [(15, 35)])], gate_ld=32)
    # activity exactly at the threshold and its two neighbours (form 0 judges speakers 0, 1, 2)
    add(8, 4, 6, 3, 16, 0, 0, 0, "random", [(0, 6, False, [(0, 24)]), (2, 4, True, [(4, 20)])], th=0.3, threshold_rows=True)
    add(8, 8, 5, 3, 17, 1, 3, 1, "random", [(0, 5, False, [(0, 24)]), (2, 3, True, [(4, 20)])], th=0.7, threshold_rows=True)
    # what a path makes of T 8, hop 4, no morphology, pushed frame by frame: 73 frames of a window of WF = 76 are transformed, the
    # seventeenth segment completes and frames [64, 68) are gated -- one block, whose lanes look at frames 64 .. 79 of a row of 76
    add(8, 4, 19, 3, 5, 0, 0, 0, "random", [(0, 17, False, [(64, 68)])], ld_min=76)
    return out


def tail_with_ring(i):
    """whether job i of a case runs with the gate ring (two of three do)"""
    return i % 3 != 2


def tail_jobs(c):
    """[(window scalars, arrays, t_lo, t_hi)] of a case, one per range"""
    jobs = []
    for wd in c["windows"]:
        w, arrs = window_inputs(c, wd)
        for lo, hi in wd["ranges"]:
            jobs.append((w, arrs, lo, hi))
    return jobs


def tail_table_jobs(n):
    """n jobs of one S and F from several cases: mixed ranges, erosions and bases, one job empty, the longest job last"""
    pool = [c for c in tail_cases() if c["S"] == 3 and c["F"] in (5, 16)]
    by_f = {}
    for c in pool:
        by_f.setdefault(c["F"], []).extend(tail_jobs(c))
    jobs = sorted(by_f[5] if len(by_f[5]) >= 6 else by_f[16], key=lambda j: j[3] - j[2])
    picked = [jobs[i % (len(jobs) - 1)] for i in range(n - 1)] + [jobs[-1]]
    w0, a0, lo0, _ = picked[3]
    picked[3] = (w0, a0, lo0, lo0)
    return picked


# ---- scatter and ingest -----------------------------------------------------------------------------------------------------------

def ingest_tile(C):
    """the launch's tile at C channels (launch_stream_ingest_pcm16_multi)"""
    return max(64, min(1024, 32768 // (2 * C) // 64 * 64))


def ingest(src, C, n, plane_ld, dst, dst_col, dst_ld, mut=None):
    """dst[dst_col + c dst_ld + i] = q[i][c] 2^-15 on the allocation dst (a copy is returned)"""
    dst = dst.copy()
    src = np.asarray(src, np.int16)
    tile = ingest_tile(C)
    for c in range(C):
        q = src[c * plane_ld:c * plane_ld + n] if plane_ld > 0 else src[c:n * C:C]
        v = q.astype(np.float32) * (f32(1.0) / f32(32767.0) if mut == "scale_32767" else f32(2.0 ** -15))
        keep = np.ones(n, bool)
        if mut == "tail_dropped" and plane_ld == 0 and C > 1:
            # the values of every tile's span behind its last whole 16 bytes never reach the LDS
            for i0 in range(0, n, tile):
                nt = min(tile, n - i0)
                j = np.arange(nt) * C + c
                keep[i0:i0 + nt] = j < (nt * C) // 8 * 8
        at = dst_col + c * dst_ld
        dst[at:at + n][keep] = v[keep]
    return dst


INGEST_VALUES = np.array([-32768, 32767, -1, 0, 1, 12345, -12345], np.int16)


def ingest_cases():
    """C x layout x n (0, 1, 7, 8, 9, 63, 64, 65 and tile - 1, tile, tile + 1, 2 tile + 3) x destination column"""
    out = []
    for C in (1, 2, 7, 8, 64):
        tile = ingest_tile(C)
        ns = [0, 1, 7, 8, 9, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 3]
        for i, n in enumerate(ns):
            for layout in ("interleaved", "planar", "planar_ld"):
                out.append(dict(name=f"C{C}_{layout}_n{n}", C=C, n=n, layout=layout, dst_col=(i + C + len(layout)) % 4, seed=40 * C + i))
    return out


def ingest_inputs(c):
    """(src int16, plane_ld, dst canaries, dst_ld): the planted values stand first and last of every tile of every channel"""
    C, n = c["C"], c["n"]
    rng = np.random.default_rng(c["seed"])
    q = rng.integers(-32768, 32768, (n, C)).astype(np.int16)
    tile = ingest_tile(C)
    for k, i in enumerate(sorted({0, n - 1, tile - 1, tile, n - 2} & set(range(n)))):
        q[i, :] = np.roll(np.resize(INGEST_VALUES, max(C, len(INGEST_VALUES))), -k)[:C]
    plane_ld = 0 if c["layout"] == "interleaved" else (n if c["layout"] == "planar" else n + 5)
    if plane_ld == 0 and c["layout"] != "interleaved":
        plane_ld = 1     # (n = 0: any positive pitch says planar)
    if c["layout"] == "interleaved":
        src = q.reshape(-1).copy()
    else:
        src = np.full(max((C - 1) * plane_ld + n, 0), CANARY16, np.int16)
        for ch in range(C):
            src[ch * plane_ld:ch * plane_ld + n] = q[:, ch]
    dst_ld = c["dst_col"] + n + 3
    return src, plane_ld, canary(c["dst_col"] + (C - 1) * dst_ld + n + 256), dst_ld


def scatter(src, src_ld, rows, e, dst):
    """columns [src_col, src_col + n_cols) of src [rows][src_ld] -> dst[dst_off + row dst_ld + c] (a copy is returned)"""
    dst = dst.copy()
    s = np.asarray(src, np.float32).reshape(-1)[:rows * src_ld].reshape(rows, src_ld)
    for r in range(rows):
        at = e["dst_off"] + r * e["dst_ld"]
        dst[at:at + e["n_cols"]] = s[r, e["src_col"]:e["src_col"] + e["n_cols"]]
    return dst


SCATTER_ROWS = (1, 3, 4, 5, 1028)
SCATTER_COLS = (0, 1, 63, 64, 65, 186, 372)
SCATTER_ENTRIES = (1, 16, 17, 33)
SCATTER_TABLES = ((1, 33), (3, 1), (4, 16), (5, 17), (1028, 17))    # (rows, entries) of the GPU test; scatter_entries(entries, rows)


def scatter_entries(n_entries, seed):
    """entries with n_cols, source columns and destination offsets rotating through the list (all residues mod 4)"""
    out = []
    for i in range(n_entries):
        n_cols = SCATTER_COLS[(i + seed) % len(SCATTER_COLS)]
        out.append(dict(n_cols=n_cols, src_col=(i * 5 + seed) % 23, dst_off=(i + seed // 2) % 4, dst_ld=n_cols + (i % 3)))
    return out


SCATTER_SRC_LD = 23 + 372 + 1


# ---- append ---------------------------------------------------------------------------------------------------------------------

def open_frames(n):
    return (n - 200) // 160 + 1 if n >= 201 else 0


def handoff_rows(dn):
    return (dn + 200) // 160 + 2 + 3


def padded_cols(xs, base, n, i, closing, mut=None):
    """columns i (an index array) of the reflect-padded concatenation of n samples, of which xs holds those from `base` on: sample j
    stands at 200 + j, reflections without edge repeat on both sides (handoff_reference.operand), the gather kernel's clamp to
    sample 0 for n < 201, zeros behind n + 400.  Open: what is known so far, zeros where a sample at or behind n would stand."""
    i = np.asarray(i, np.int64)
    if n == 0:
        return np.zeros(len(i), np.float32)
    j = np.abs(i - 200)
    zero = (i >= n + 400) if closing else (j >= n)
    if closing:
        j = np.where(j >= n, 2 * (n - 1) - j + (1 if mut == "right_edge_repeat" else 0), j)
        if mut == "no_clamp":
            zero |= j < 0
        j = np.maximum(j, 0)
    at = j - base
    ok = ~zero & (at >= 0) & (at < len(xs))
    return np.where(ok, np.asarray(xs, np.float32)[np.clip(at, 0, max(len(xs) - 1, 0))] if len(xs) else f32(0), f32(0)).astype(np.float32)


def append_round(job, k, mut=None):
    """speaker k of one job of launch_handoff_append_multi, from the job's inputs alone: gate [S][gate_ld] (the ring), out
    [S][out_ld], carry_in [S][carry_ld], tail_in [S][512], st [S] and the scalars -> dict with A1, J1, n_new, rows, operand
    [rows 160] with `defined` (the columns that hold defined values), tail (the samples tail_out holds from tail_at on),
    carry (carry_out's samples), act (act_out's bytes)"""
    g = lambda name: int(job[name])
    pad, drop, closing = g("pad"), g("drop"), g("closing")
    t_g0, t_g1, D0, D1, out_base, mask = g("t_g0"), g("t_g1"), g("D0"), g("D1"), g("out_base"), g("gate_ld") - 1
    ring, out, carry_in, tail_in = job["gate"][k], job["out"][k], job["carry_in"][k], job["tail_in"][k]
    A0, J0 = int(job["st"][k]["A"]), int(job["st"][k]["J"])
    tail0 = 160 * J0 - 200 if J0 > 0 else 0

    def sample(n):
        if n >= out_base:
            return out[n - out_base] if n - out_base < len(out) else f32(0)
        return carry_in[(n - out_base) % len(carry_in)] if mut == "carry_from_out_base" else carry_in[n - D0]

    passes, cur = [], []
    q_lo, q_hi = D0 // 256, -(-D1 // 256)
    for q in range(q_lo, q_hi):
        if (q - q_lo) % 256 == 0 and q > q_lo:
            passes.append(cur)
            cur = []
        keep = not drop
        if drop:
            lo = max(q - pad - (0 if mut == "keep_lo_off" else 1), 0)
            hi = q + pad + (1 if mut == "keep_hi_off" else 0)
            if mut != "keep_past_tg1":
                hi = min(hi, t_g1 - 1)
            keep = any(ring[t & mask] != 0 for t in range(lo, hi + 1))
        if keep:
            end = (q + 1) * 256 if mut == "last_block_uncut" else min((q + 1) * 256, D1)
            cur.extend(sample(n) for n in range(q * 256, end))
    passes.append(cur)
    if mut == "second_pass_restarts" and len(passes) > 1:
        new = list(passes[0])
        for p in passes[1:]:
            new[:len(p)] = p
        new = new[:len(passes[-1])]
    else:
        new = [v for p in passes for v in p]
    # the concatenation as far as the round knows it: the tail's samples from max(tail0, 0) on, then the new ones
    base = max(tail0, 0)
    xs = np.concatenate([tail_in[base - tail0:A0 - tail0], np.array(new, np.float32)]).astype(np.float32)
    A1 = A0 + len(new)
    as_closing = (closing and mut != "J_open_on_closing") or (not closing and mut == "J_closing_on_open")
    J1 = A1 // 160 if as_closing else open_frames(A1)
    rows = handoff_rows(D1 - D0)
    op = padded_cols(xs, base, A1, 160 * J0 + np.arange(rows * 160), closing, mut)
    n_new = J1 - J0
    tail1 = 160 * J1 - 200 if J1 > 0 else 0
    tail_at = 160 * J0 if mut == "tail_from_J0" else max(tail1, 0)
    return dict(A1=A1, J1=J1, n_new=n_new, rows=rows, operand=op, defined=min(max(160 * (n_new - 1) + 400, 0) if n_new > 0 else 0, rows * 160),
                tail=xs[tail_at - base:][:TAIL_LD], tail_at=tail_at - tail1, carry=np.array([sample(n) for n in range(D1, 256 * t_g1)], np.float32),
                act=np.array([ring[t & mask] for t in range(t_g0, t_g1)], np.uint8), xs=xs, base=base)


def append_gate(kind, TL, pad):
    """the recording's gate bytes [TL]"""
    g = np.zeros(TL, np.uint8)
    if kind == "pauses":        # runs with pauses of exactly 2 pad + 1, 2 pad + 2 and 2 pad + 3 frames (merged, touching, apart)
        t = 3
        for gap in (2 * pad + 1, 2 * pad + 2, 2 * pad + 3, 2 * pad + 2):
            if t + 2 >= TL:
                break
            g[t:t + 2] = 1
            t += 2 + gap
        if t + 2 < TL:
            g[t:t + 2] = 1
    elif kind == "all_active":
        g[:] = 1
    elif kind == "frame_0":
        g[0] = 1
    elif kind == "frame_last":
        g[TL - 1] = 1
    elif kind == "both_ends":
        g[0] = g[TL - 1] = 1
    elif kind != "silent":
        raise ValueError(kind)
    return g


def append_cuttings(TL, pad, how):
    """the gated-final frame counts after each open round; the closing round follows them"""
    if how == "all_at_once":
        return []
    step = {"every_frame": 1, "7": 7, "16": 16, "100": 100}[how]
    return list(range(step, TL, step))


def append_cases():
    """pad x drop x gate x cutting, rotated: every pad meets every gate kind and every cutting at least once"""
    out = []
    kinds = ("pauses", "silent", "all_active", "frame_0", "frame_last", "both_ends")
    cuts = ("every_frame", "7", "16", "100", "all_at_once")
    i = 0
    for pad in (0, 1, 3, 8):
        for gi, kind in enumerate(kinds):
            TL = 12 * pad + 40 + gi
            out.append(dict(name=f"pad{pad}_{kind}_{cuts[i % 5]}", pad=pad, drop=1, kind=kind, TL=TL, n_out=(TL + 1) * 256 - (37 if i % 2 else 0),
                            cut=cuts[i % 5], seed=300 + i, S=3))
            i += 1
    for pad, kind, cut in ((0, "pauses", "16"), (8, "pauses", "every_frame"), (3, "silent", "7")):
        out.append(dict(name=f"nodrop_pad{pad}_{kind}_{cut}", pad=pad, drop=0, kind=kind, TL=45, n_out=46 * 256 - 100, cut=cut, seed=300 + i, S=3))
        i += 1
    # pad 300: the closing round decides more than 256 blocks (pad + T + ...), one speaker all active, one silent, one at the ends
    out.append(dict(name="pad300_closing_pass2", pad=300, drop=1, kind="both_ends", TL=330, n_out=331 * 256 - 11, cut="100", seed=390, S=3,
                    kinds=("all_active", "both_ends", "frame_last")))
    # one open round deciding more than 256 blocks, the second pass keeping samples behind a pause
    out.append(dict(name="open_pass2", pad=1, drop=1, kind="pauses", TL=300, n_out=301 * 256, cut="open_290", seed=391, S=3,
                    kinds=("all_active", "pass2_only", "pass2_late")))
    # closing with a total of 150 samples (below 201: the clamped reflection, frames = 0) by an n_out that cuts the only kept block,
    # of exactly one block (256: one frame), and of nothing
    out.append(dict(name="closing_150", pad=0, drop=1, kind="frame_last", TL=20, n_out=19 * 256 + 150, cut="7", seed=392, S=3,
                    kinds=("frame_last", "silent", "frame_last")))
    out.append(dict(name="closing_180", pad=0, drop=1, kind="frame_last", TL=20, n_out=19 * 256 + 180, cut="all_at_once", seed=394, S=3,
                    kinds=("frame_last", "silent", "frame_last")))
    out.append(dict(name="closing_256", pad=0, drop=1, kind="frame_last", TL=20, n_out=20 * 256, cut="16", seed=393, S=3,
                    kinds=("frame_last", "frame_last", "silent")))
    for c in out:
        # the smallest ring that holds every round's look-back (64 at least), the carry of pad blocks and a little more
        pad = c["pad"] if c["drop"] else 0
        look = max(t1 - (min(t0, max(D0 // 256 - pad - 1, 0)) if c["drop"] else t0) for t0, t1, D0, _, _ in append_rounds(c))
        c["gate_ld"] = max(64, 1 << (look - 1).bit_length())
        c["carry_ld"] = pad * 256 + 8 + max(256 * c["TL"] - c["n_out"], 0)
    return out


def append_recording(c):
    """(wav [S][n_out + 512] float32, gate [S][TL]); speaker k's gate kind rotates from the case's"""
    if "_rec" in c:
        return c["_rec"]
    S, TL = c["S"], c["TL"]
    rng = np.random.default_rng(c["seed"])
    wav = rng.uniform(-1, 1, (S, c["n_out"] + 512)).astype(np.float32)
    wav[wav == 0] = 0.5
    kinds = ("pauses", "silent", "all_active", "frame_0", "frame_last", "both_ends")
    gate = np.zeros((S, TL), np.uint8)
    for k in range(S):
        kind = c["kinds"][k] if "kinds" in c else kinds[(kinds.index(c["kind"]) + 2 * k) % len(kinds)]
        if kind == "pass2_only":
            gate[k, 270:275] = 1
        elif kind == "pass2_late":
            gate[k, 10:14] = 1
            gate[k, 262:264] = 1
        else:
            gate[k] = append_gate(kind, TL, c["pad"])
    c["_rec"] = (wav, gate)
    return c["_rec"]


def append_rounds(c):
    """[(t_g0, t_g1, D0, D1, closing)] as handoff_round makes them: D1 = max(t_g1 - pad, 0) 256 while open, n_out when closing"""
    TL, pad = c["TL"], c["pad"] if c["drop"] else 0
    cuts = [290] if c["cut"] == "open_290" else append_cuttings(TL, pad, c["cut"])
    rounds, t_g, D = [], 0, 0
    for t1 in cuts:
        D1 = max(t1 - pad, 0) * 256
        rounds.append((t_g, t1, D, D1, 0))
        t_g, D = t1, D1
    rounds.append((t_g, TL, D, c["n_out"], 1))
    return rounds


def ring_of(gate, t_g1, gate_ld, junk):
    """the ring after the gate kernel finalised frames below t_g1: frame t at t & (gate_ld - 1) for the last gate_ld frames, `junk`
    bytes (what stale frames and frames not gated-final leave there) elsewhere"""
    S = gate.shape[0]
    ring = np.full((S, gate_ld), junk, np.uint8)
    for t in range(max(t_g1 - gate_ld, 0), t_g1):
        ring[:, t & (gate_ld - 1)] = gate[:, t]
    return ring


def append_job(c, rnd, state, junk=1, nan_unread=True, out_lead=0):
    """the job of one round of a case: state = (carry [S][carry_ld], tail [S][512], st [S]) from the round before.  Samples the
    round does not read (dropped blocks, `out` before out_base's decided part) are NaN; ring bytes of frames the round may not look
    at are `junk`."""
    wav, gate = append_recording(c)
    t_g0, t_g1, D0, D1, closing = rnd
    S = c["S"]
    carry, tail, st = state
    carry_ld = carry.shape[1]
    out_base = t_g0 * 256
    end = max(D1, 256 * t_g1)
    out = wav[:, out_base:end].copy()
    job = dict(pad=c["pad"] if c["drop"] else 0, drop=c["drop"], closing=closing, S=S, gate_ld=c["gate_ld"], out_ld=out.shape[1], out_base=out_base,
               carry_ld=carry_ld, t_g0=t_g0, t_g1=t_g1, D0=D0, D1=D1, gate=ring_of(gate, t_g1, c["gate_ld"], junk), out=out, carry_in=carry,
               tail_in=tail, st=st)
    if nan_unread:
        # what the definition keeps of [D0, D1): everything else of it is never read
        for k in range(S):
            keep = np.zeros(end, bool)
            for a, b in H.kept_ranges(gate[k], job["pad"], D1, bool(c["drop"])):
                keep[a:b] = True
            keep[D1:] = True
            dead = ~keep[out_base:end]
            job["out"][k, dead] = np.nan
            cdead = ~keep[D0:min(out_base, end)]
            ci = job["carry_in"].copy() if k == 0 else job["carry_in"]
            ci[k, :len(cdead)][cdead] = np.nan
            job["carry_in"] = ci
    return job


def append_state0(S, carry_ld, A0=0, tail=None):
    """the state before the first round (or a later one: A0 samples appended, `tail` [S][<= 400] their last samples from
    160 J0 - 200 on)"""
    st = np.zeros(S, STATE)
    st["A"], st["J"], st["gmax"], st["pad"] = A0, open_frames(A0), GMAX_NONE, 0
    t = np.full((S, TAIL_LD), np.nan, np.float32)
    if tail is not None:
        t[:, :tail.shape[1]] = tail
    return np.full((S, carry_ld), np.nan, np.float32), t, st


def append_definition(c, k):
    """speaker k of the whole recording: (concatenation, frames n // 160, padded operand [n + 400]) by handoff_reference"""
    wav, gate = append_recording(c)
    x = H.concat(wav[k], H.kept_ranges(gate[k], c["pad"] if c["drop"] else 0, c["n_out"], bool(c["drop"])))
    return x, H.frames_of(len(x)), padded_cols(x, 0, len(x), np.arange(len(x) + 400), True)


# ---- mel ------------------------------------------------------------------------------------------------------------------------

def order_int(v):
    """the order-preserving integer form of float32 values (handoff_mel_tile)"""
    b = np.asarray(v, np.float32).view(np.int32)
    return np.where(b >= 0, b, b ^ np.int32(0x7FFFFFFF))


def mel_reference(spec, ld, col0, nfr, n_mels):
    """float64 log-mel of the float32 spectra spec [402][ld] at columns col0 .. col0 + nfr: (raw [n_mels][nfr], bound on it, floor:
    where the device value is -10.0f bit for bit): handoff_reference.bound with the product's terms set to zero"""
    r = H.Ref()
    s = np.asarray(spec, np.float32).reshape(402, ld)[:, col0:col0 + nfr].astype(np.float64)
    r.re, r.im = s[:H.BINS], s[H.BINS:]
    r.power = r.re * r.re + r.im * r.im
    r.W = H.tables(n_mels)[1]
    r.mel = r.W @ r.power
    r.raw = np.log10(np.maximum(r.mel, H.FLOOR))
    r.mx = r.raw.max()
    r.out = (np.maximum(r.raw, r.mx - 8.0) + 4.0) / 4.0
    r.s_re = r.s_im = np.zeros_like(r.re)
    H.bound(r, k_prod=0)
    floor = r.mel + r.e_mel <= H.FLOOR
    return r.raw, r.e_raw, floor


def mel_side(mel, n_new, rows, J, gmax_in, hist, mut=None):
    """what the launch derives from the float32 mel [n_mels][mel_ld] it wrote for one speaker: (gmax after, frame maxima [nfr],
    {slot: frame j} of the history)"""
    nfr = min(n_new, rows)
    if nfr == 0:
        return np.int32(gmax_in), np.zeros(0, np.float32), {}
    v = mel[:, :nfr]
    if mut == "signed_bits_max":
        top = max(int(np.int32(gmax_in)), int(v.view(np.int32).max()))
    else:
        top = max(int(np.int32(gmax_in)), int(order_int(v).max()))
    fm = v.max(axis=0)
    slots = {}
    if hist:
        js = range(min(nfr, hist)) if mut == "first_hist_kept" else range(max(nfr - hist, 0), nfr)
        for j in js:
            slots[(j if mut == "slot_without_count" else J - n_new + j) % hist] = j
    return np.int32(top), fm, slots


def mel_spectra(kind, nfr, seed):
    """[402][nfr] float32: a handoff_reference signal through the float64 DFT of its frames, rounded once; zeros; one subnormal bin"""
    if kind == "zeros":
        return np.zeros((402, nfr), np.float32)
    if kind == "subnormal":
        s = np.zeros((402, nfr), np.float32)
        s[37, :] = f32(2.0 ** -140)
        s[201 + 90, ::2] = f32(2.0 ** -130)
        return s
    x = H.signal(kind, 160 * nfr + 400, seed=seed)
    fr = np.lib.stride_tricks.sliding_window_view(x.astype(np.float64), H.NFFT)[::H.HOPW][:nfr].T
    return (H.tables(80)[0] @ fr).astype(np.float32)


MEL_KINDS = ("noise", "tones", "chirp", "quiet_chirp", "square", "zeros", "subnormal")


def mel_cases():
    """jobs of S = 3 speakers: n_new per speaker out of 0, 1, 31, 32, 33, rows, rows + 5; gmax presets; history and pvmax forms"""
    out = []
    presets = ("reset", "below", "above")
    for i, (n_mels, rows, n_new) in enumerate(((80, 40, (0, 1, 31)), (128, 40, (32, 33, 40)), (80, 33, (38, 0, 33)), (128, 35, (1, 35, 32)))):
        out.append(dict(name=f"plain_{n_mels}_{i}", n_mels=n_mels, rows=rows, n_new=n_new, form="plain", hist=0, J=(0, 0, 0), seed=600 + i,
                        presets=tuple(presets[(i + k) % 3] for k in range(3)), kinds=tuple(MEL_KINDS[(2 * i + k) % len(MEL_KINDS)] for k in range(3))))
    for i, (n_mels, rows, n_new, hist, J) in enumerate((
            (80, 40, (33, 8, 7), 8, (33 + 7, 2 ** 32 + 5, 16)), (128, 40, (33, 1, 0), 8, (2 ** 32 + 8 * 3 + 1, 8, 77)),
            (80, 36, (36, 31, 40), 50, (49 + 36, 50, 2 ** 33 + 45)), (128, 34, (5, 34, 9), 16, (5, 34 + 15, 16)))):
        out.append(dict(name=f"hist_{n_mels}_{i}", n_mels=n_mels, rows=rows, n_new=n_new, form="ring", hist=hist, J=J, seed=620 + i,
                        presets=tuple(presets[(i + k + 1) % 3] for k in range(3)), kinds=tuple(MEL_KINDS[(3 * i + k + 1) % len(MEL_KINDS)] for k in range(3))))
    for i, (n_mels, rows, n_new) in enumerate(((80, 40, (33, 0, 40)), (128, 33, (1, 32, 38)))):
        out.append(dict(name=f"pvmax_{n_mels}_{i}", n_mels=n_mels, rows=rows, n_new=n_new, form="pvmax", hist=0, J=(0, 0, 0), seed=640 + i,
                        presets=tuple(presets[(i + k + 2) % 3] for k in range(3)), kinds=tuple(MEL_KINDS[(i + 2 * k) % len(MEL_KINDS)] for k in range(3))))
    return out


def mel_case_spec(c, row0, ld, spec):
    """writes the case's spectra into spec [402][ld] at its columns (the columns behind n_new stay as they are: NaN)"""
    for k in range(3):
        nfr = min(c["n_new"][k], c["rows"])
        if nfr:
            spec[:, row0 + k * c["rows"]:row0 + k * c["rows"] + nfr] = mel_spectra(c["kinds"][k], nfr, c["seed"] + k)


# ---- what the tests assert of a round, and the state it leaves ---------------------------------------------------------------------

def append_asserted(r):
    """the elements of a round's model that the GPU test holds the launch to, as one list of arrays"""
    return [np.array([r["A1"], r["J1"], r["n_new"]], np.int64), bits(r["operand"][:r["defined"]]), bits(r["tail"]), np.array([r["tail_at"]]),
            bits(r["carry"]), r["act"]]


def append_next(job, results):
    """(carry, tail, st) for the round after `job`, from the models of its speakers: the arrays as the launch leaves them, NaN where
    it writes nothing"""
    S = job["S"]
    carry = np.full((S, job["carry_ld"]), np.nan, np.float32)
    tail = np.full((S, TAIL_LD), np.nan, np.float32)
    st = job["st"].copy()
    for k, r in enumerate(results):
        carry[k, :len(r["carry"])] = r["carry"]
        tail[k, r["tail_at"]:r["tail_at"] + len(r["tail"])] = r["tail"]
        st[k]["A"], st[k]["J"] = r["A1"], r["J1"]
    return carry, tail, st


def append_chain(c, rounds=None, mut=None, on_round=None):
    """the rounds of a case through the model (the state always the definition's); on_round(job, results, mutated results or None)"""
    state = append_state0(c["S"], c["carry_ld"])
    for rnd in (append_rounds(c) if rounds is None else rounds):
        job = append_job(c, rnd, state)
        res = [append_round(job, k) for k in range(c["S"])]
        if on_round is not None:
            on_round(job, res, None if mut is None else [append_round(job, k, mut) for k in range(c["S"])])
        state = append_next(job, res)
    return state


BIG = 2 ** 32


def append_big_state(S=3, seed=77):
    """a start state with A0 and J0 beyond 2^32 and the matching tail, an open round of 20 frames and the closing one behind it:
    (case, state, rounds).  The recording's frames and samples count from 0 in the job; only the state is far out."""
    c = dict(name="big_state", pad=1, drop=1, kind="pauses", TL=40, n_out=41 * 256 - 5, cut="big", seed=seed, S=S, gate_ld=64, carry_ld=256 + 8)
    rng = np.random.default_rng(seed)
    st = np.zeros(S, STATE)
    tail = np.full((S, TAIL_LD), np.nan, np.float32)
    for k in range(S):
        A0 = BIG * (k + 1) + 160 * 7 + (33, 0, 159)[k % 3] + 200
        st[k]["A"], st[k]["J"], st[k]["gmax"] = A0, open_frames(A0), GMAX_NONE
        n = A0 - (160 * int(st[k]["J"]) - 200)
        tail[k, :n] = rng.uniform(-1, 1, n).astype(np.float32)
    rounds = [(0, 20, 0, 19 * 256, 0), (20, 40, 19 * 256, c["n_out"], 1)]
    return c, (np.full((S, c["carry_ld"]), np.nan, np.float32), tail, st), rounds
