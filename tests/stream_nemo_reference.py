"""An exact numpy model of one round of the streamed NeMo hand-off's append (csrc/nemo_stream.hip nemo_append_kernel;
include/css_mi355_stream_nemo.h): a job's inputs -- the gate ring, the round's samples, the carry, the tail, the counts and the
last kept sample -- in, the speaker's operand rows and the state the round leaves out.  No GPU, no library:
tests/test_stream_nemo_reference.py proves on the CPU that rounds of the model compose to tests/nemo_reference.py's operand of the
whole recording, tests/test_hip_stream_nemo_kernels.py holds the kernel to the model bit for bit.

The definition: A kept samples appended so far, y their pre-emphasised concatenation (y[0] = x[0], y[c] = x[c] - p x[c - 1] with
the product and the difference rounded to float32 apart; x[c - 1] is the last kept sample before, across a seam and across a
round); frame j reads y[160 j - 256, 160 j + 256) with zeros below 0; an open stream has J = (A - 256) // 160 + 1 frames once
A >= 256, a closing round A // 160 with zeros from y[A] on.  Operand column x of a round is y[160 J0 - 256 + x]; the tail a round
leaves is y[160 J1 - 256, A1) with zeros where that lies before the recording's start.

The gate ring, the block rule, the decided samples, the carry and the gate bytes are the Whisper append's: the cases, recordings,
rounds and jobs are tests/stream_reference.py's (append_cases, append_recording, append_rounds, append_job), with more below for
what only this format has.  `mut` names one deliberate mistake (MISTAKES); None is the definition."""
import numpy as np

import handoff_reference as H
import nemo_reference as N
import stream_reference as SR
from frontend_reference import bits  # noqa: F401

f32 = np.float32
TAIL_LD = 512                           # NEMO_TAIL_LD
LEAD = 256                              # samples of y a frame reads beyond its hop's start

MISTAKES = ("preemph_restart_round", "preemph_restart_seam", "xlast_from_y", "whisper_frame_rule", "tail_400", "tail_start_not_zero",
            "no_closing_zeros")


def open_frames(A, mut=None):
    if mut == "whisper_frame_rule":
        return (A - 200) // 160 + 1 if A >= 201 else 0
    return (A - LEAD) // 160 + 1 if A >= LEAD else 0


def nemo_rows(dn):
    return (dn + LEAD) // 160 + 2 + 4


def append_round(job, k, mut=None):
    """speaker k of one job of launch_nemo_append_multi, from the job's inputs alone: SR.append_round's inputs with tail_in
    [S][512] = y[160 J0 - 256, A0), xlast_in [S] and preemphasis -> dict with A1, J1, n_new, rows, operand [rows 160] (every column
    defined), tail (tail_out's floats from 0 on), carry, act, xlast, ranges (the sample ranges the round appended)"""
    g = lambda name: int(job[name])
    pad, drop, closing = g("pad"), g("drop"), g("closing")
    t_g0, t_g1, D0, D1, out_base, mask = g("t_g0"), g("t_g1"), g("D0"), g("D1"), g("out_base"), g("gate_ld") - 1
    ring, out, carry_in, tail_in = job["gate"][k], job["out"][k], job["carry_in"][k], job["tail_in"][k]
    A0, J0 = int(job["st"][k]["A"]), int(job["st"][k]["J"])
    p = f32(job["preemphasis"])

    def sample(n):
        return out[n - out_base] if n >= out_base else carry_in[n - D0]

    new, seams, ranges = [], [], []
    for q in range(D0 // 256, -(-D1 // 256)):
        keep = not drop
        if drop:
            keep = any(ring[t & mask] != 0 for t in range(max(q - pad - 1, 0), min(q + pad, t_g1 - 1) + 1))
        if not keep:
            continue
        a, b = q * 256, min((q + 1) * 256, D1)
        if ranges and ranges[-1][1] == a:
            ranges[-1][1] = b
        else:
            ranges.append([a, b])
            seams.append(len(new))                                  # the first sample behind a seam (or the round's first)
        new.extend(sample(n) for n in range(a, b))
    x = np.array(new, np.float32)
    y = x.copy()
    if p != 0 and len(x):
        before = np.concatenate([[f32(job["xlast_in"][k])], x[:-1]]).astype(np.float32)
        prod = (p * before).astype(np.float32)                      # rounded once
        y = (x - prod).astype(np.float32)                           # and the difference once
        if A0 == 0:
            y[0] = x[0]                                             # concatenation sample 0 has no predecessor
        if mut == "preemph_restart_round":
            y[0] = x[0]
        if mut == "preemph_restart_seam":
            y[seams] = x[seams]
    A1 = A0 + len(x)
    J1 = A1 // 160 if closing else open_frames(A1, mut)
    rows = nemo_rows(D1 - D0)
    base = 160 * J0 - LEAD
    c = base + np.arange(rows * 160)
    op = np.zeros(rows * 160, np.float32)
    old = (c >= 0) & (c < A0)
    if mut == "tail_start_not_zero":
        old = c < A0
    if mut == "tail_400":
        old &= (c - base) < 400
    op[old] = tail_in[(c - base)[old]]
    mine = (c >= A0) & (c < A1)
    op[mine] = y[(c - A0)[mine]]
    if mut == "no_closing_zeros" and closing:
        op[c >= A1] = np.nan                                        # (whatever an earlier round left there)
    tail1 = 160 * J1 - LEAD
    tc = np.arange(tail1, A1)[:400 if mut == "tail_400" else TAIL_LD]
    tail = np.zeros(len(tc), np.float32)
    inside = tc >= 0
    tail[inside] = op[(tc - base)[inside]]
    if len(x) == 0:
        xlast = f32(job["xlast_in"][k])
    else:
        xlast = y[-1] if mut == "xlast_from_y" else x[-1]
    return dict(A1=A1, J1=J1, n_new=J1 - J0, rows=rows, operand=op, tail=tail,
                carry=np.array([sample(n) for n in range(D1, 256 * t_g1)], np.float32),
                act=np.array([ring[t & mask] for t in range(t_g0, t_g1)], np.uint8), xlast=np.float32(xlast), ranges=ranges)


# ---- cases ------------------------------------------------------------------------------------------------------------------------

def _case(name, pad, drop, gates, TL, n_out, cuts, seed, p=0.97):
    """a case in SR.append_cases()' form with explicit gate rows `gates` [S][TL] and open rounds ending at the frames `cuts`"""
    c = dict(name=name, pad=pad, drop=drop, kind="explicit", TL=TL, n_out=n_out, cut="explicit", cuts=list(cuts), seed=seed, S=len(gates),
             preemphasis=p)
    rng = np.random.default_rng(seed)
    wav = rng.uniform(-1, 1, (len(gates), n_out + 512)).astype(np.float32)
    wav[wav == 0] = 0.5
    c["_rec"] = (wav, np.asarray(gates, np.uint8))
    return _sized(c)


def _sized(c):
    pad = c["pad"] if c["drop"] else 0
    look = max(t1 - (min(t0, max(D0 // 256 - pad - 1, 0)) if c["drop"] else t0) for t0, t1, D0, _, _ in rounds_of(c))
    c["gate_ld"] = max(64, 1 << (look - 1).bit_length())
    c["carry_ld"] = pad * 256 + 8 + max(256 * c["TL"] - c["n_out"], 0)
    return c


def rounds_of(c):
    """[(t_g0, t_g1, D0, D1, closing)] as handoff_round makes them (SR.append_rounds; a round may repeat t_g: it appends nothing)"""
    if c["cut"] != "explicit":
        return SR.append_rounds(c)
    pad = c["pad"] if c["drop"] else 0
    rounds, t_g, D = [], 0, 0
    for t1 in c["cuts"]:
        D1 = max(t1 - pad, 0) * 256
        rounds.append((t_g, t1, D, D1, 0))
        t_g, D = t1, D1
    rounds.append((t_g, c["TL"], D, c["n_out"], 1))
    return rounds


def _gate(TL, *runs):
    g = np.zeros(TL, np.uint8)
    for a, b in runs:
        g[a:b] = 1
    return g


def named_cases():
    """the cases the format adds, by what they are there for (pad 0 unless named: block q is kept iff frame q - 1 or q is active)"""
    TL = 40
    never = _gate(TL)
    out = [
        # speaker 0: blocks [4, 8) and [12, 16) kept -- the second run's first block is the first block of the round that starts at
        # D = 12 * 256 (cut at frame 12): a seam exactly on a round boundary; speaker 1 never active; speaker 2 always
        _case("seam_on_round_boundary", 0, 1, [_gate(TL, (4, 7), (12, 15)), never, _gate(TL, (0, TL))], TL, 41 * 256, (4, 8, 12, 20), 500),
        # cuts that repeat (t_g does not move: nothing is appended) and rounds inside a pause
        _case("round_appends_nothing", 0, 1, [_gate(TL, (2, 4), (30, 33)), never, _gate(TL, (10, 11))], TL, 41 * 256 - 9, (6, 6, 10, 20, 20, 35), 501),
        # A crosses 256 inside a round: one kept block (256 samples) then more in the same round
        _case("A_crosses_256_in_round", 0, 1, [_gate(TL, (3, 5), (9, 10)), _gate(TL, (0, 1), (20, 22)), never], TL, 41 * 256, (30,), 502),
        # a recording whose only kept block is cut by n_out to 100 samples: A < 160, no frame ever
        _case("A_below_160", 0, 1, [_gate(20, (19, 20)), _gate(20), _gate(20, (19, 20))], 20, 19 * 256 + 100, (7, 14), 503),
        # ... to 200 samples: 160 <= A < 256, one frame, at finish only
        _case("A_160_to_256", 0, 1, [_gate(20, (19, 20)), _gate(20), _gate(20, (19, 20))], 20, 19 * 256 + 200, (7, 14), 504),
        # the same shapes without pre-emphasis, and with padding 3 / no drop
        _case("p_zero", 0, 1, [_gate(TL, (4, 7), (12, 15)), never, _gate(TL, (0, TL))], TL, 41 * 256 - 77, (4, 8, 12, 20), 505, p=0.0),
        _case("pad3_seams", 3, 1, [_gate(TL, (2, 3), (14, 15), (30, 31)), never, _gate(TL, (20, 21))], TL, 41 * 256 - 5, (5, 11, 17, 18, 29), 506),
        _case("nodrop", 8, 0, [_gate(TL, (2, 3)), never, _gate(TL, (0, TL))], TL, 41 * 256 - 300, (1, 2, 9, 25), 507),
    ]
    return out


def cases():
    """SR.append_cases() (pads 0, 1, 3, 8, 300, drop on and off, six gates, five cuttings, rounds of more than 256 blocks, closing
    at 150 / 180 / 256 samples) with p = 0.97 and, every third, p = 0; then the named ones"""
    out = []
    for i, c in enumerate(SR.append_cases()):
        c = dict(c, preemphasis=0.0 if i % 3 == 2 else 0.97)
        c.pop("_rec", None)
        out.append(c)
    return out + named_cases()


def random_cases(n=24, seed=2027):
    """random gates (runs of 1 .. 6 frames with pauses of 1 .. 25), pads 0 / 3 / 8, drop on and off, random cuttings"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        pad, drop = (0, 3, 8)[i % 3], 0 if i % 4 == 3 else 1
        TL = int(rng.integers(30, 90))
        gates = []
        for k in range(3):
            g, t = np.zeros(TL, np.uint8), int(rng.integers(0, 12))
            while t < TL and k != i % 5:            # (k == i % 5: a speaker never active)
                on = int(rng.integers(1, 7))
                g[t:t + on] = 1
                t += on + int(rng.integers(1, 26))
            gates.append(g)
        cuts = sorted(int(v) for v in rng.integers(1, TL, int(rng.integers(1, 9))))
        n_out = (TL + 1) * 256 - int(rng.integers(0, 256)) * (i % 2)
        out.append(_case(f"random_{i}_pad{pad}_drop{drop}", pad, drop, gates, TL, n_out, cuts, 600 + i, p=0.97 if i % 6 else 0.0))
    return out


# ---- rounds, states, the definition -------------------------------------------------------------------------------------------------

def state0(c):
    """(carry, tail, st, xlast) before the first round: NaN where nothing may be read"""
    carry, tail, st = SR.append_state0(c["S"], c["carry_ld"])
    st["gmax"] = 0
    return carry, tail, st, np.full(c["S"], np.nan, np.float32)


def job_of(c, rnd, state, junk=1):
    """SR.append_job (samples the round never reads are NaN, ring bytes it may not look at are `junk`) with this format's inputs"""
    job = SR.append_job(c, rnd, state[:3], junk=junk)
    job["preemphasis"], job["xlast_in"] = c["preemphasis"], state[3]
    return job


def next_state(job, results):
    S = job["S"]
    carry = np.full((S, job["carry_ld"]), np.nan, np.float32)
    tail = np.full((S, TAIL_LD), np.nan, np.float32)
    st = job["st"].copy()
    xlast = np.zeros(S, np.float32)
    for k, r in enumerate(results):
        carry[k, :len(r["carry"])] = r["carry"]
        tail[k, :len(r["tail"])] = r["tail"]
        st[k]["A"], st[k]["J"] = r["A1"], r["J1"]
        xlast[k] = r["xlast"]
    return carry, tail, st, xlast


def chain(c, mut=None):
    """all rounds of a case through the model, the state always the model's own (a mistake feeds itself) -> per speaker
    (frames [J][512] emitted in order, merged ranges, A, J)"""
    S = c["S"]
    state = state0(c)
    rows = [[] for _ in range(S)]
    ranges = [[] for _ in range(S)]
    for rnd in rounds_of(c):
        job = job_of(c, rnd, state)
        res = [append_round(job, k, mut) for k in range(S)]
        for k, r in enumerate(res):
            for j in range(max(r["n_new"], 0)):
                rows[k].append(r["operand"][160 * j:160 * j + 512].copy())
            for a, b in r["ranges"]:
                if ranges[k] and ranges[k][-1][1] == a:
                    ranges[k][-1][1] = b
                else:
                    ranges[k].append([a, b])
        state = next_state(job, res)
    return [(np.array(rows[k], np.float32).reshape(-1, 512), np.array(ranges[k], np.int64).reshape(-1, 2), int(state[2][k]["A"]),
             int(state[2][k]["J"])) for k in range(S)]


def definition(c, k):
    """speaker k of the whole recording by tests/nemo_reference.py and tests/handoff_reference.py: (kept ranges, the operand rows
    [A // 160][512] of the zero-padded pre-emphasised concatenation, the concatenation)"""
    wav, gate = SR.append_recording(c)
    ranges = np.array(H.kept_ranges(gate[k], c["pad"] if c["drop"] else 0, c["n_out"], bool(c["drop"])), np.int64).reshape(-1, 2)
    y = N.preemphasised(wav[k], ranges, c["preemphasis"])
    nfr = N.frames_of(len(y))
    op = N.padded(y).astype(np.float32)
    fr = np.lib.stride_tricks.sliding_window_view(op, 512)[::160][:nfr] if nfr else np.zeros((0, 512), np.float32)
    return ranges, np.ascontiguousarray(fr, np.float32), N.concat(wav[k], ranges)


# which listed case each named mistake must break (tests/test_stream_nemo_reference.py asserts it)
CAUGHT_BY = {
    "preemph_restart_round": "seam_on_round_boundary",
    "preemph_restart_seam": "pad3_seams",
    "xlast_from_y": "seam_on_round_boundary",
    "whisper_frame_rule": "seam_on_round_boundary",
    "tail_400": "A_crosses_256_in_round",
    "tail_start_not_zero": "A_crosses_256_in_round",
    "no_closing_zeros": "A_160_to_256",
}
