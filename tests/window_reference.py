"""Exact models of the window kernels and the queued sessions' hand-off kernels of csrc/handoff.hip -- session_keep_scan_kernel,
session_gather_kernel, session_norm_kernel, session_window_kernel, stream_window_kernel -- the case lists of
tests/test_hip_window_kernels.py and the named mistakes as `mut` switches (DESIGN.md 7b "The window and session hand-off kernels,
launch form by launch form").  No GPU, no library: tests/test_window_reference.py checks this file on the CPU.

All five kernels are exact functions of their inputs (counts, copies, fmaxf, one float32 subtraction, one addition, one
multiplication by 0.25, one round-to-nearest-even to float16), so every model gives every output bit:
  scan     a gate byte is active iff nonzero; an active frame t keeps the sample blocks t - pad .. t + pad + 1 that lie in 0 .. TL
           (block q is kept iff a frame of [q - pad - 1, q + pad] inside the row is active); without `drop` every block is kept.
           The runs are the maximal kept runs in ascending order, in samples; offs[r] = the kept samples before run r;
           A = 256 (kept blocks), J = A // 160, gmax = 0x80808080; psum[t] = active frames below t, written only with drop.
           Only the first cap_ranges runs are tabulated; the counts are the true ones.
  gather   operand element i of speaker k is sample reflect(i - 200) of the speaker's concatenation for i < A + 400 where A > 0
           and a run is tabulated, 0 otherwise; 416 zeros follow the last speaker's rows.  The concatenation is read through the
           table: sample j belongs to the last tabulated run r with offs[r] <= j and is wav[regs[r][0] + j - offs[r]] -- so with
           more runs than the table holds, the samples behind the last tabulated run are that run's continuation in wav.
  norm / windows   the rule of include/css_mi355_window.h: (fmax(raw, M - 8) + 4) / 4 in float32 with fmaxf's NaN rule (np.fmax: a
           NaN frame takes the clamp's floor), fill = (fmax(-10, M - 8) + 4) / 4, float16 = astype.  A session's M is decoded from
           gmax's order-preserving integer form; a stream window's M is the fmax over the per-frame maxima of its span.
  stream span   P = min(*n_new, pv_ld) (0 without provisional frames), E = J + P, R = max(J - hist, 0), a = max(E - n_frames, R),
           used = E - a, n_provisional = min(used, P), p0 = P - n_provisional: ring frames [a, J) at slots f mod hist, then
           provisional frames p0 .. P - 1.
Everything a launch does not own keeps the canary: the models start from the caller's arrays and write only what is owned.

`mut` names one deliberate mistake (SCAN_MISTAKES, GATHER_MISTAKES, NORM_MISTAKES, WINDOW_MISTAKES, STREAM_MISTAKES); None is the
definition.  The mistakes that concern how a kernel walks its data (chunks, words, 16-byte groups) are switches of scan_walk and
row_walk, which restate the walk; tests/test_window_reference.py holds both to the definitions on every case."""
import numpy as np

from frontend_reference import CANARY, bits, canary  # noqa: F401  (shared with the other kernel tests)

f32 = np.float32
CANARY_BYTE = np.uint8(0xA5)
CANARY16 = np.uint16(0x5A5A)
CANARY32 = np.int32(0x5A5A5A5A)
CANARY64 = np.int64(0x5A5A5A5A5A5A5A5A)
STATE = np.dtype([("A", "<i8"), ("J", "<i8"), ("gmax", "<i4"), ("pad", "<i4")])
RES = np.dtype([("first_frame", "<i8"), ("n_used", "<i4"), ("n_provisional", "<i4"), ("window_max", "<f4"), ("pad", "<i4")])
GMAX_RESET = np.int32(-2139062144)      # 0x80808080
CHUNK = 1024                            # SESSION_SCAN_CHUNK
WHOLE_CHUNK = 4096                      # SESSION_WINDOW_CHUNK
TABLE = 32                              # WINDOW_MULTI_MAX
SLACK = 256                             # canaries behind every output of the GPU test
INF = f32(np.inf)

SCAN_MISTAKES = ("keep_shifted", "clamp_at_TL", "carry_dropped", "alignment_ignored", "runs_restart", "end_to_r", "offs_in_blocks",
                 "J_plus_one", "no_cap_guard")
GATHER_MISTAKES = ("left_edge_repeat", "right_edge_repeat", "first_region", "no_zero_tail")
NORM_MISTAKES = ("no_xor", "column_J_written")
WINDOW_MISTAKES = ("no_xor", "fill_minus_1_5", "last_group_vector", "select_off_by_one", "f16_truncated", "chunk_start_dropped",
                   "J_unclamped")
# A head counted in bytes for float16 moves the boundary between scalar and 16-byte stores and nothing else: every column still
# takes its own value (tests/test_window_reference.py proves it on every case), so no output bit can show it; what it would do is
# store 16 bytes off a 16-byte boundary.
WINDOW_MISTAKES_UNREAD = ("head_in_bytes",)
STREAM_MISTAKES = ("slot0_from_J", "no_wrap", "p0_zero", "ring_max_only", "P_unclamped", "a_without_floor")


def canary_state(n):
    return np.full(int(n) * 6, CANARY32, np.int32).view(STATE).copy()


def canary_res(n):
    return np.full(int(n) * 6, CANARY32, np.int32).view(RES).copy()


def decode_max(gmax, mut=None):
    """the float32 a state row's gmax stands for (order-preserving integer form, stream_reference.order_int)"""
    b = np.int32(gmax)
    if b < 0 and mut != "no_xor":
        b = b ^ np.int32(0x7FFFFFFF)
    return np.array([b], np.int32).view(np.float32)[0]


def encode_max(v):
    b = np.array([v], np.float32).view(np.int32)[0]
    return b if b >= 0 else b ^ np.int32(0x7FFFFFFF)


def norm(raw, M):
    with np.errstate(invalid="ignore"):
        return (np.fmax(np.asarray(raw, f32), f32(M) - f32(8.0)) + f32(4.0)) * f32(0.25)


def fill_of(M, mut=None):
    return f32(-1.5) if mut == "fill_minus_1_5" else norm(f32(-10.0), M)


def to_f16(v, mut=None):
    """float32 -> float16 words"""
    v = np.asarray(v, f32)
    h = v.astype(np.float16)
    if mut == "f16_truncated":
        with np.errstate(invalid="ignore", over="ignore"):
            over = np.isfinite(v) & (np.abs(h.astype(f32)) > np.abs(v))
        h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.view(np.uint16)


# ---- the keep-scan ------------------------------------------------------------------------------------------------------------------

def path_cap(TL, pad, drop=1):
    """the capacity below which the path refuses (api_session_handoff.hip session_bounds)"""
    return (TL - 1) // (2 * pad + 3) + 1 if drop else 1


def kept_blocks(active, pad, drop=1):
    """active [TL] bool -> kept [TL + 1] bool"""
    TL = len(active)
    kept = np.zeros(TL + 1, bool)
    if not drop:
        kept[:] = True
        return kept
    for t in np.flatnonzero(active):
        kept[max(t - pad, 0):min(t + pad + 1, TL) + 1] = True
    return kept


def runs_of(kept):
    """maximal runs of a bool row: [n][2] (first, behind the last)"""
    k = np.concatenate([[False], kept, [False]]).astype(np.int8)
    d = np.diff(k)
    return np.stack([np.flatnonzero(d == 1), np.flatnonzero(d == -1)], axis=1).astype(np.int64)


def scan_blank(c):
    S, TL, cap = c["S"], c["TL"], c["cap_ranges"]
    i64, i32 = (lambda n: np.full(n + SLACK, CANARY64, np.int64)), (lambda n: np.full(n + SLACK, CANARY32, np.int32))
    return dict(psum=i32(S * (TL + 1)), regs=i64(S * cap * 2), offs=i64(S * cap), st=canary_state(S + SLACK), n_new=i32(S), n_ranges=i32(S),
                ranges_out=i64(S * cap * 2), n_frames_out=i64(S), n_ranges_out=i32(S))


def scan(c, blank=None, mut=None):
    """the keep-scan of case c (S, TL, pad, drop, cap_ranges, gate_off, gate: the allocation, gate_off bytes in front) on copies of
    the arrays of `blank` (scan_blank)"""
    if mut in SCAN_MISTAKES:
        return scan_walk(c, blank, mut)
    assert mut is None
    S, TL, pad, cap = c["S"], c["TL"], c["pad"], c["cap_ranges"]
    o = {k: v.copy() for k, v in (blank or scan_blank(c)).items()}
    for k in range(S):
        row = c["gate"][c["gate_off"] + k * TL:c["gate_off"] + (k + 1) * TL]
        active = row != 0
        if c["drop"]:
            o["psum"][k * (TL + 1):(k + 1) * (TL + 1)] = np.concatenate([[0], np.cumsum(active)])
        kept = kept_blocks(active, pad, c["drop"])
        runs = runs_of(kept)
        before = np.concatenate([[0], np.cumsum(kept)])
        for r, (a, b) in enumerate(runs[:cap]):
            o["regs"][(k * cap + r) * 2:(k * cap + r) * 2 + 2] = (256 * a, 256 * b)
            o["ranges_out"][(k * cap + r) * 2:(k * cap + r) * 2 + 2] = (256 * a, 256 * b)
            o["offs"][k * cap + r] = 256 * before[a]
        A = 256 * int(kept.sum())
        o["st"]["A"][k], o["st"]["J"][k], o["st"]["gmax"][k] = A, A // 160, GMAX_RESET
        o["n_new"][k] = o["n_frames_out"][k] = A // 160
        o["n_ranges"][k] = o["n_ranges_out"][k] = len(runs)
    return o


def scan_walk(c, blank=None, mut=None):
    """the same results by the kernel's walk -- prefix sums in chunks of 1024 laid over the 32-bit words of the row, then kept flags,
    run indices and kept-block counts in chunks of 1024 blocks -- with the mistakes of SCAN_MISTAKES as switches.  Bytes behind the
    row are the allocation's own (the next row, then the slack)."""
    S, TL, pad, cap, off = c["S"], c["TL"], c["pad"], c["cap_ranges"], c["gate_off"]
    o = {k: v.copy() for k, v in (blank or scan_blank(c)).items()}
    mem = np.concatenate([c["gate"], np.full(8, CANARY_BYTE, np.uint8)])

    def put(name, i, v):                     # a store into the allocation, slack included
        if 0 <= i < len(o[name]):
            o[name][i] = v

    for k in range(S):
        base = off + k * TL
        a = base & 3
        t = np.arange(TL)
        src = t.copy()
        if mut == "alignment_ignored":       # whole words are read `a` bytes further up
            u = (t + a) // 4 * 4
            whole = (u >= a) & (u + 4 <= a + TL)
            src = np.where(whole, t + a, t)
        active = mem[base + src] != 0
        psum = np.concatenate([[0], np.cumsum(active)]).astype(np.int64)
        if mut == "carry_dropped":           # every chunk of 1024 frames (laid over the words) counts from 0
            ch = (t + a) // CHUNK
            psum[1:] -= np.concatenate([[0], np.cumsum(np.bincount(ch, weights=active))]).astype(np.int64)[ch]
        if mut == "clamp_at_TL":             # (frame TL is the byte behind the row; psum goes one further)
            psum = np.concatenate([psum, [psum[-1] + int(mem[base + TL] != 0)]])
        if c["drop"]:
            o["psum"][k * (TL + 1):(k + 1) * (TL + 1)] = psum[:TL + 1]
        q = np.arange(TL + 1)
        if not c["drop"]:
            kept = np.ones(TL + 1, bool)
        else:
            lo, hi = q - pad - 1, q + pad
            if mut == "keep_shifted":
                lo, hi = lo + 1, hi + 1
            top = TL if mut == "clamp_at_TL" else TL - 1
            kept = psum[np.minimum(hi, top) + 1] - psum[np.maximum(lo, 0)] > 0
        start = kept & ~np.concatenate([[False], kept[:-1]])
        end = kept & ~np.concatenate([kept[1:], [False]])
        blocks = np.concatenate([[0], np.cumsum(kept)])
        r = np.cumsum(start)                 # run starts at or below q
        if mut == "runs_restart":            # every chunk of 1024 blocks counts its runs from 0
            r = r - np.concatenate([[0], np.cumsum(np.bincount(q // CHUNK, weights=start))]).astype(np.int64)[q // CHUNK]
        for qq in np.flatnonzero(start):
            i = int(r[qq]) - 1
            if i < cap or mut == "no_cap_guard":
                put("regs", (k * cap + i) * 2, 256 * qq)
                put("ranges_out", (k * cap + i) * 2, 256 * qq)
                put("offs", k * cap + i, (1 if mut == "offs_in_blocks" else 256) * blocks[qq])
        for qq in np.flatnonzero(end):
            i = int(r[qq]) - (0 if mut == "end_to_r" else 1)
            if (0 <= i < cap) or (mut == "no_cap_guard" and i >= 0):
                put("regs", (k * cap + i) * 2 + 1, 256 * (qq + 1))
                put("ranges_out", (k * cap + i) * 2 + 1, 256 * (qq + 1))
        A = 256 * int(kept.sum())
        J = A // 160 + (1 if mut == "J_plus_one" else 0)
        o["st"]["A"][k], o["st"]["J"][k], o["st"]["gmax"][k] = A, J, GMAX_RESET
        o["n_new"][k] = o["n_frames_out"][k] = J
        o["n_ranges"][k] = o["n_ranges_out"][k] = int(start.sum())
    return o


GATE_KINDS = ("none", "all", "first", "last", "gap_merge", "gap_split", "edges_1024", "bytes", "sparse", "dense")
PADS = (0, 1, 3, 300, 4096)
SCAN_TLS = tuple(range(1, 6)) + tuple(range(1019, 1030)) + tuple(range(2047, 2051)) + (3073,)


def gate_row(kind, TL, pad, a, seed):
    """one row of gate bytes; `a` is the row's byte alignment (the chunks of pass 1 end at frames 1024 c - a)"""
    g = np.zeros(TL, np.uint8)
    rng = np.random.default_rng(seed)
    if kind == "all":
        g[:] = 1
    elif kind == "first":
        g[0] = 1
    elif kind == "last":
        g[TL - 1] = 1
    elif kind in ("gap_merge", "gap_split"):       # pairs of active frames 2 pad + 1 (the blocks touch) / 2 pad + 2 frames apart
        gap = 2 * pad + (1 if kind == "gap_merge" else 2)
        t = int(rng.integers(0, 3))
        while t < TL:
            g[t] = 1
            if t + gap + 1 < TL:
                g[t + gap + 1] = 1
            t += 2 * gap + 4 * pad + 9
    elif kind == "edges_1024":                     # a run that ends or starts at frame 1023 / 1024 / 1025 of every chunk of frames,
        runs = (((-5, 0), (1, 4)), ((-4, 1),), ((-1, 3),), ((0, 4),), ((-3, 2),))   # and of every chunk of words from the second on
        for n, c0 in enumerate(range(CHUNK, TL + 4, CHUNK)):
            for lo, hi in runs[(seed + n) % 5]:
                shift = a if n else 0
                g[max(c0 + lo - shift, 0):max(min(c0 + hi - shift, TL), 0)] = 1
        g[max(TL - 1 - (seed % 3), 0)] = 1
    elif kind == "bytes":
        g[:] = rng.choice(np.array([0, 0, 0, 0x80, 0xFF, 2], np.uint8), TL)
    elif kind == "sparse":
        g[:] = rng.random(TL) < 0.02
    elif kind == "dense":
        g[:] = rng.random(TL) < 0.5
    return g


def _scan_case(name, S, TL, pad, drop, gate_off, kinds, seed, cap=None):
    rows = [gate_row(kinds[k % len(kinds)], TL, pad, (gate_off + k * TL) & 3, seed + k) for k in range(S)]
    gate = np.concatenate([np.full(gate_off, CANARY_BYTE, np.uint8)] + rows + [np.full(SLACK, CANARY_BYTE, np.uint8)])
    c = dict(name=name, S=S, TL=TL, pad=pad, drop=drop, gate_off=gate_off, gate=gate, kinds=[kinds[k % len(kinds)] for k in range(S)])
    counts = [len(runs_of(kept_blocks(r != 0, pad, drop))) for r in rows]
    c["counts"] = counts
    c["cap_ranges"] = path_cap(TL, pad, drop) if cap is None else max(cap(max(counts)), 1)
    return c


_SCAN_CASES = []


def scan_cases():
    """every TL x gate_off with S, pad and the gate kinds rotating; runs at the chunk edges for every row alignment; capacities at
    and below the run count; drop off"""
    if _SCAN_CASES:
        return _SCAN_CASES
    out, i = [], 0
    for TL in SCAN_TLS:
        for gate_off in range(4):
            S, pad = 1 + (i + gate_off) % 4, PADS[i % 5]
            kinds = GATE_KINDS[i % len(GATE_KINDS):] + GATE_KINDS[:i % len(GATE_KINDS)]
            out.append(_scan_case(f"scan_TL{TL}_off{gate_off}_S{S}_pad{pad}_{kinds[0]}", S, TL, pad, 1, gate_off, kinds, 100 + i))
            i += 1
    for TL in (1029, 2050, 3073):
        for gate_off in range(4):
            for pad in (0, 1):
                out.append(_scan_case(f"scan_edges_TL{TL}_off{gate_off}_pad{pad}", 4, TL, pad, 1, gate_off, ("edges_1024",), 7 * TL + gate_off + pad))
    for TL in (5, 1027):
        for pad in PADS:
            for kind in ("gap_merge", "gap_split", "none", "all", "first", "last", "bytes"):
                out.append(_scan_case(f"scan_{kind}_TL{TL}_pad{pad}", 2, TL, pad, 1, 1, (kind,), TL + pad))
    for TL, kind in ((1029, "dense"), (3073, "sparse"), (2049, "edges_1024"), (5, "gap_split")):
        for what, cap in (("exact", lambda n: n), ("minus_1", lambda n: n - 1), ("one", lambda n: 1)):
            for S in (1, 3):
                out.append(_scan_case(f"scan_cap_{what}_TL{TL}_{kind}_S{S}", S, TL, 0, 1, S, (kind, "sparse", "dense"), 900 + TL, cap))
    for TL in (1, 4, 1025, 2049):
        out.append(_scan_case(f"scan_nodrop_TL{TL}", 3, TL, 1, 0, TL & 3, ("sparse", "none", "all"), 50 + TL))
    _SCAN_CASES.extend(out)
    return out


# ---- the gather ---------------------------------------------------------------------------------------------------------------------

def path_rows(TL):
    """operand rows per speaker on the path (api_session_handoff.hip layout): n_out / 160 + 3 for the n_out = 256 (TL + 1) samples"""
    return 256 * (TL + 1) // 160 + 3


def concatenation(wav_row, regs, offs, n_ranges, cap, A, mut=None):
    """the A samples the table stands for (regs [cap][2], offs [cap]): run r gives the samples [offs[r], offs[r + 1]), the last
    tabulated run everything from offs[r] on"""
    nr = min(int(n_ranges), cap)
    if A <= 0 or nr <= 0:
        return np.zeros(0, f32)
    if mut == "first_region":
        nr = 1
    x = np.empty(A, f32)
    for r in range(nr):
        lo = 0 if r == 0 else int(offs[r])
        hi = A if r == nr - 1 else min(int(offs[r + 1]), A)
        if hi > lo:
            s = int(regs[r][0]) + lo - int(offs[r])
            x[lo:hi] = wav_row[s:s + hi - lo]
    return x


def reflect_padded(x, mut=None):
    """x reflect-padded by 200 at both ends, no edge repeat; below 201 samples the index stops at sample 0"""
    A = len(x)
    j = np.arange(A + 400) - 200
    j = np.where(j < 0, -j - (1 if mut == "left_edge_repeat" else 0), j)
    j = np.where(j >= A, 2 * (A - 1) - j + (1 if mut == "right_edge_repeat" else 0), j)
    return x[np.clip(j, 0, A - 1)]


def gather(c, operand, mut=None):
    """the gather of case c (S, cap_ranges, wav_off, wav_ld, rows, regs, offs, st, n_ranges, wav: the allocation) into a copy of
    `operand` (S rows 160 + 416 floats)"""
    S, cap, per = c["S"], c["cap_ranges"], c["rows"] * 160
    out = operand.copy()
    regs, offs = c["regs"][:S * cap * 2].reshape(S, cap, 2), c["offs"][:S * cap].reshape(S, cap)
    for k in range(S):
        n = per + (416 if k == S - 1 and mut != "no_zero_tail" else 0)
        A = int(c["st"]["A"][k])
        x = concatenation(c["wav"][c["wav_off"] + k * c["wav_ld"]:c["wav_off"] + (k + 1) * c["wav_ld"]], regs[k], offs[k], c["n_ranges"][k], cap, A, mut)
        row = np.zeros(n, f32)
        if len(x):
            v = reflect_padded(x, mut)[:n]
            row[:len(v)] = v
        out[k * per:k * per + n] = row
    return out


_GATHER_CASES = []


def _gather_case(name, S, cap, wav_off, wav_ld, rows, regs, offs, A, n_ranges, seed):
    st = canary_state(S)
    st["A"], st["J"] = A, np.asarray(A) // 160
    rng = np.random.default_rng(seed)
    wav = np.concatenate([np.full(wav_off, np.nan, f32), rng.standard_normal(S * wav_ld).astype(f32), np.full(8, np.nan, f32)])
    return dict(name=name, S=S, cap_ranges=cap, wav_off=wav_off, wav_ld=wav_ld, rows=rows, regs=np.asarray(regs, np.int64).reshape(-1),
                offs=np.asarray(offs, np.int64).reshape(-1), st=st, n_ranges=np.asarray(n_ranges, np.int32), wav=wav)


def gather_cases():
    """the tables the scan model gives for a spread of the scan cases (the over-capacity ones among them), rows as on the path and
    one more; hand-made tables with A of 256 and 512, A = 0, no run, and equal offs"""
    if _GATHER_CASES:
        return _GATHER_CASES
    out = []
    picked = [c for i, c in enumerate(scan_cases()) if i % 6 == 0 or "_cap_" in c["name"] or "nodrop" in c["name"]]
    for i, c in enumerate(picked):
        o = scan(c)
        S, cap, TL = c["S"], c["cap_ranges"], c["TL"]
        regs, offs = o["regs"][:S * cap * 2].copy(), o["offs"][:S * cap].copy()
        for k in range(S):                                   # (rows of the table no run reached: not read; keep them harmless)
            n = min(int(o["n_ranges"][k]), cap)
            regs[(k * cap + n) * 2:(k + 1) * cap * 2] = 0
            offs[k * cap + n:(k + 1) * cap] = 0
        g = _gather_case("gather_" + c["name"], S, cap, i % 4, 256 * (TL + 1) + 3, path_rows(TL) + (i & 1), regs, offs,
                         o["st"]["A"][:S].copy(), o["n_ranges"][:S].copy(), 300 + i)
        out.append(g)
    for A, wav_off in ((256, 1), (512, 2), (1, 3), (201, 0)):
        out.append(_gather_case(f"gather_A{A}", 2, 2, wav_off, 700, 6, [[100, 100 + A], [0, 0], [5, 5 + A], [0, 0]], [0, 0, 0, 0], [A, A], [1, 1], A))
    out.append(_gather_case("gather_empty", 3, 2, 1, 600, 5, [[0, 512], [0, 0]] * 3, [0, 0] * 3, [0, 512, 512], [1, 0, 1], 11))
    out.append(_gather_case("gather_equal_offs", 1, 3, 2, 900, 6, [[10, 266], [300, 300], [400, 656]], [0, 256, 256], [512], [3], 12))
    _GATHER_CASES.extend(out)
    return out


# ---- the normalisation --------------------------------------------------------------------------------------------------------------

def session_norm(c, out, mut=None):
    """c: S, n_mels, mel_ld, out_ld, rows, st, mel (flat) -> a copy of `out` with the columns below min(J, out_ld) written"""
    S, nm, mel_ld, out_ld = c["S"], c["n_mels"], c["mel_ld"], c["out_ld"]
    o = out.copy()
    if c["rows"] <= 0:
        return o
    mel = c["mel"][:S * nm * mel_ld].reshape(S, nm, mel_ld)
    body = o[:S * nm * out_ld].reshape(S, nm, out_ld)
    for k in range(S):
        n = int(c["st"]["J"][k]) + (1 if mut == "column_J_written" else 0)
        n = min(n, out_ld, mel_ld)
        body[k, :, :n] = norm(mel[k, :, :n], decode_max(c["st"]["gmax"][k], mut))
    o[:S * nm * out_ld] = body.reshape(-1)
    return o


def mel_rows(S, nm, mel_ld, Js, maxima, seed, lead=0, quiet=False):
    """raw log-mel rows: values at most the speaker's maximum below J (the maximum itself among them), +inf from J on"""
    rng = np.random.default_rng(seed)
    mel = np.full((S, nm, mel_ld), INF, f32)
    for k in range(S):
        J = min(int(Js[k]), mel_ld)
        v = f32(maxima[k]) - (rng.random((nm, J)) * (4 if quiet else 14)).astype(f32)
        if J:
            v[rng.integers(nm), rng.integers(J)] = maxima[k]
        mel[k, :, :J] = v
    return np.concatenate([np.full(lead, INF, f32), mel.reshape(-1), np.full(8, INF, f32)])


def state_rows(Js, maxima):
    st = canary_state(len(Js))
    st["J"], st["A"] = Js, np.asarray(Js, np.int64) * 160
    st["gmax"] = [encode_max(m) for m in maxima]
    return st


def norm_cases():
    out = []
    for i, (Js, rows, out_ld) in enumerate((((0, 1, 255, 256), 256, 300), ((257, 300, 256, 0), 300, 256), ((257, 1, 255, 300), 300, 200),
                                            ((3, 0, 2, 1), 3, 5), ((600, 513, 512, 511), 600, 600), ((5, 5), 0, 8))):
        S = len(Js)
        maxima = [(1.5, -2.25, 0.0, -0.0078125)[(k + i) % 4] for k in range(S)]
        nm, mel_ld = (5, 8, 9)[i % 3], rows + 3
        Jc = [min(J, max(rows, 0)) for J in Js]
        out.append(dict(name=f"norm_{i}_J{'_'.join(map(str, Js))}_rows{rows}_ld{out_ld}", S=S, n_mels=nm, mel_ld=mel_ld, out_ld=out_ld, rows=rows,
                        st=state_rows(Jc, maxima), mel=mel_rows(S, nm, mel_ld, Jc, maxima, 40 + i)))
    return out


# ---- a row as the window kernels write it -------------------------------------------------------------------------------------------

def row_walk(src, src_at, row_len, s0, n, wd, dst_at, el, M, mut=None):
    """columns 0 .. wd - 1 of a window row: normalised src[src_at + s0 + c] for c < n, the fill behind -- by the kernel's walk:
    scalar columns up to the destination's first 16-byte boundary (dst_at: the row's first element, counted in elements of `el`
    bytes from a 256-byte boundary), groups of 16 bytes from there, scalar columns behind the last whole group; a group wholly
    below n is loaded 16 bytes at a time from a source of any alignment (src_at + s0 + c floats from such a boundary).  float32."""
    V = 16 // el
    fill = fill_of(M, mut)
    head = ((16 - (dst_at * el) % 16) % 16) // (1 if mut == "head_in_bytes" else el)
    head = min(head, wd)
    nvec = (wd - head) // V
    out = np.empty(wd, f32)

    def get(i):
        return src[i] if 0 <= i < len(src) else INF

    def one(c):
        return norm(get(src_at + s0 + c), M) if c < n else fill

    for c in list(range(head)) + list(range(head + nvec * V, wd)):
        out[c] = one(c)
    for g in range(nvec):
        c = head + g * V
        vec, shift = c + V <= n or (mut == "last_group_vector" and c < n), 0
        if vec:
            s = s0 + c
            d = (src_at + s) & 3
            if d and not (s >= d and s - d + V + 4 <= row_len):
                vec = mut == "last_group_vector"
            shift = 1 if (mut == "select_off_by_one" and d and vec) else 0
        for i in range(V):
            out[c + i] = norm(get(src_at + s0 + c + i + shift), M) if vec else one(c + i)
    return out


# ---- session windows ----------------------------------------------------------------------------------------------------------------

def session_windows_blank(c):
    S, nm = c["S"], c["n_mels"]
    cn = (lambda n: np.full(n, CANARY16, np.uint16)) if c["f16"] else (lambda n: canary(n).copy())
    o = dict(n_windows_out=np.full(S + SLACK, CANARY32, np.int32), window_max_out=canary(S + SLACK).copy())
    if c.get("cap_windows"):
        o["win"] = cn(c["win_off"] + S * c["cap_windows"] * nm * c["ld"] + SLACK)
    if c.get("whole_ld"):
        o["whole"] = cn(c["whole_off"] + S * nm * c["whole_ld"] + SLACK)
    return o


def session_windows(c, blank=None, mut=None):
    """c: S, n_mels, width, stride, f16, mel_off, mel_ld, max_frames, st, mel (the allocation) and, where the output is asked for,
    win_off, ld, cap_windows / whole_off, whole_ld -> copies of `blank`'s arrays (session_windows_blank) as the launch leaves them"""
    S, nm, width, stride, mel_ld = c["S"], c["n_mels"], c["width"], c["stride"], c["mel_ld"]
    o = {k: v.copy() for k, v in (blank or session_windows_blank(c)).items()}
    el = 2 if c["f16"] else 4
    cast = (lambda v: to_f16(v, mut)) if c["f16"] else (lambda v: v)
    walk = mut in ("last_group_vector", "select_off_by_one", "head_in_bytes", "walk")
    n_win_jobs = -(-c["max_frames"] // stride) if "win" in o else 0

    def row(k, m, s0, n, wd, dst_at, M):
        at = c["mel_off"] + (k * nm + m) * mel_ld
        if walk:
            return row_walk(c["mel"], at, mel_ld, s0, n, wd, dst_at, el, M, mut)
        v = np.full(wd, fill_of(M, mut), f32)
        have = c["mel"][at + s0:at + s0 + n]
        v[:len(have)] = norm(have, M)
        v[len(have):n] = norm(INF, M)        # (reads behind the allocation: a mistake's)
        return v

    for k in range(S):
        J = int(c["st"]["J"][k])
        if mut != "J_unclamped":
            J = min(J, c["max_frames"])
        M = decode_max(c["st"]["gmax"][k], mut)
        o["n_windows_out"][k] = -(-J // stride)
        o["window_max_out"].view(np.uint32)[k] = np.array([M], f32).view(np.uint32)[0]
        if J <= 0:
            continue
        for m in range(nm):
            for w in range(n_win_jobs):
                n = min(J - w * stride, width)
                if n < 1:
                    break
                at = c["win_off"] + ((k * c["cap_windows"] + w) * nm + m) * c["ld"]
                o["win"][at:at + width] = cast(row(k, m, w * stride, n, width, at, M))
            if "whole" in o:
                for s0 in range(0, c["whole_ld"], WHOLE_CHUNK):
                    wd = min(c["whole_ld"] - s0, WHOLE_CHUNK)
                    at = c["whole_off"] + (k * nm + m) * c["whole_ld"] + (0 if mut == "chunk_start_dropped" else s0)
                    o["whole"][at:at + wd] = cast(row(k, m, s0, max(min(J - s0, wd), 0), wd, at, M))
    return o


def _sw_case(name, S, nm, width, stride, f16, Js, max_frames, mel_off=0, win_off=0, whole_off=0, ld_extra=0, win=True, whole_ld=0, maxima=None,
             seed=0, mel_ld=None):
    maxima = maxima or [(1.5, -2.25, 0.0, 0.75)[k % 4] for k in range(S)]
    mel_ld = mel_ld or max_frames + 1 + seed % 3
    c = dict(name=name, S=S, n_mels=nm, width=width, stride=stride, f16=int(f16), mel_off=mel_off, mel_ld=mel_ld, max_frames=max_frames,
             st=state_rows(Js, maxima), mel=mel_rows(S, nm, mel_ld, [min(J, max_frames) for J in Js], maxima, 60 + seed, mel_off),
             win_off=win_off, whole_off=whole_off, ld=width + ld_extra, cap_windows=0, whole_ld=whole_ld)
    if win:
        c["cap_windows"] = max(-(-max_frames // stride), 1) + seed % 2
    return c


_SW_CASES = []


def session_window_cases():
    if _SW_CASES:
        return _SW_CASES
    out, i = [], 0
    for mel_off in range(4):                       # every source alignment x destination head x dtype
        for win_off in range(8):
            for f16 in (0, 1):
                out.append(_sw_case(f"sw_align_mel{mel_off}_win{win_off}_f16{f16}", 3, 5, 64, 7, f16, (45, 23, 0), 45, mel_off, win_off,
                                    (3 * win_off + 1) % 8, i % 4, True, 50, seed=i))
                i += 1
    for width, stride in ((96, 64), (64, 7), (5, 5), (9, 1), (3000, 3000)):
        for part, Js in enumerate(((0, 1, 3, stride - 1), (stride, stride + 1, 2 * stride + 40, 3))):
            for f16 in (0, 1):
                mf = stride + 20
                out.append(_sw_case(f"sw_{width}x{stride}_J{part}_f16{f16}", 4, (8, 9)[f16], width, stride, f16, Js, mf, i % 4, i % 8, 0, i % 4, seed=i))
                i += 1
    for j, whole_ld in enumerate((0, 4095, 4096, 4097, 8197)):   # frames across the chunk boundary of `whole`
        for part, Js in enumerate(((4090, 4091, 4092, 4093), (4094, 4095, 4096, 4097), (4098, 4099, 4100, 0))):
            if whole_ld == 0 and part:
                continue
            f16 = (j + part) & 1
            out.append(_sw_case(f"sw_whole{whole_ld}_J{part}_f16{f16}", 4, 5, 96, 64, f16, Js, 4100, i % 4, i % 8, (i + 3) % 8, 0, win=whole_ld == 0 or part == 1,
                                whole_ld=whole_ld, seed=i))
            i += 1
    for f16 in (0, 1):                             # whole_ld = J exactly; n_mels 80 and 128 once each
        out.append(_sw_case(f"sw_wholeJ_f16{f16}", 2, 5, 9, 1, f16, (37, 37), 37, 1, 2, 5, 1, whole_ld=37, seed=i))
        out.append(_sw_case(f"sw_mels{(80, 128)[f16]}", 2, (80, 128)[f16], 64, 7, f16, (30, 12), 33, 2, 3, 1, 2, whole_ld=40, seed=i + 1))
        i += 2
    out.extend(tie_cases_session())
    _SW_CASES.extend(out)
    return out


def tie_cases_session():
    """float16 ties, a NaN frame inside the span, a negative maximum above every frame"""
    out = []
    for f16 in (0, 1):
        c = _sw_case(f"sw_ties_f16{f16}", 1, 5, 16, 16, f16, (12,), 12, 1, 1, 0, 0, whole_ld=20, maxima=[8.0], seed=3)
        mel = c["mel"][1:1 + 5 * c["mel_ld"]].reshape(5, c["mel_ld"])
        mel[:, :12] = 0.0
        mel[0, :4] = (2.0 ** -9, 3 * 2.0 ** -9, 8.0, np.nan)    # 1 + 2^-11 -> 1.0; 1 + 3 x 2^-11 -> 1 + 2^-9; the maximum; NaN -> the floor
        mel[3, 8:12] = (2.0 ** -9, 3 * 2.0 ** -9, 5 * 2.0 ** -9, np.nan)
        out.append(c)
        out.append(_sw_case(f"sw_negative_max_f16{f16}", 2, 5, 16, 5, f16, (14, 9), 14, 2, 3, 0, 1, whole_ld=16, maxima=[-3.96875, -20.5], seed=4))
    return out


# ---- stream windows -----------------------------------------------------------------------------------------------------------------

def span(it, n_new=None, mut=None):
    """(a, used, n_provisional, p0, P) of an item"""
    hist, J = it["hist"], it["J"]
    P = 0
    if it.get("pv") is not None:
        n_new = int(it["n_new"][0]) if n_new is None else n_new
        P = n_new if mut == "P_unclamped" else min(n_new, it["pv_ld"])
    E, R = J + P, (0 if mut == "a_without_floor" else max(J - hist, 0))
    a = max(E - it["n_frames"], R)
    used = E - a
    n_prov = min(used, P)
    return a, used, n_prov, (0 if mut == "p0_zero" else P - n_prov), P


def stream_window(it, out, res_row, mut=None):
    """one item (n_frames, width, n_mels, f16, hist, ld, J, ring_off, out_off, ring, fmax and, with provisional frames, pv_off, pv_ld,
    pv, pvmax, n_new: the allocations) -> (a copy of `out` as the launch leaves it, the result row)"""
    nm, hist, width = it["n_mels"], it["hist"], it["width"]
    a, used, n_prov, p0, P = span(it, mut=mut)
    o, r = out.copy(), res_row.copy()
    r["first_frame"], r["n_used"], r["n_provisional"] = a, used, n_prov
    if used == 0:
        return o, r
    n_ring = used - n_prov
    slots = (it["J"] if mut == "slot0_from_J" else a) % hist + np.arange(n_ring)
    if mut != "no_wrap":
        slots = slots % hist

    def take(arr, idx):                              # (a mistake may read behind the allocation)
        idx = np.asarray(idx, np.int64)
        ok = (idx >= 0) & (idx < len(arr))
        return np.where(ok, arr[np.clip(idx, 0, len(arr) - 1)], INF)

    maxima = [take(it["fmax"], slots)]
    if n_prov and mut != "ring_max_only":
        maxima.append(take(it["pvmax"], p0 + np.arange(n_prov)))
    M = np.fmax.reduce(np.concatenate([[-INF]] + maxima).astype(f32))
    r["window_max"] = M
    for m in range(nm):
        raw = take(it["ring"], it["ring_off"] + m * hist + slots)
        if n_prov:
            raw = np.concatenate([raw, take(it["pv"], it["pv_off"] + m * it["pv_ld"] + p0 + np.arange(n_prov))])
        v = np.full(width, fill_of(M), f32)
        v[:min(used, width)] = norm(raw[:width], M)
        at = it["out_off"] + m * it["ld"]
        o[at:at + width] = to_f16(v) if it["f16"] else v
    return o, r


def stream_item(name, hist, J, n_frames, width, f16=0, nm=5, n_new=None, pv_ld=0, ring_off=0, pv_off=0, out_off=0, ld_extra=0, seed=0, M=1.5,
                nan_at=None):
    """an item whose span holds values at most M (M itself among them) and whose every other frame, maximum slot and provisional
    column is +inf"""
    rng = np.random.default_rng(seed)
    it = dict(name=name, hist=hist, J=J, n_frames=n_frames, width=width, f16=int(f16), n_mels=nm, ring_off=ring_off, out_off=out_off,
              ld=width + ld_extra, pv_ld=pv_ld, pv_off=pv_off)
    if n_new is not None:
        it["n_new"] = np.array([n_new], np.int32)
        it["pv"] = np.zeros(0, f32)
    a, used, n_prov, p0, P = span(it)
    ring = np.full((nm, hist), INF, f32)
    fmax = np.full(hist, INF, f32)
    slots = (a + np.arange(used - n_prov)) % hist
    vals = f32(M) - (rng.random((nm, used)) * 14).astype(f32)
    if used:
        vals[rng.integers(nm), rng.integers(used)] = M
    if nan_at is not None and used:
        vals[nan_at[0] % nm, nan_at[1] % used] = np.nan
    colmax = np.fmax.reduce(vals, axis=0) if used else np.zeros(0, f32)
    ring[:, slots] = vals[:, :len(slots)]
    fmax[slots] = colmax[:len(slots)]
    it["ring"] = np.concatenate([np.full(ring_off, INF, f32), ring.reshape(-1), np.full(8, INF, f32)])
    it["fmax"] = fmax
    if n_new is not None:
        pv, pvmax = np.full((nm, pv_ld), INF, f32), np.full(pv_ld, INF, f32)
        pv[:, p0:P] = vals[:, len(slots):]
        pvmax[p0:P] = colmax[len(slots):]
        it["pv"] = np.concatenate([np.full(pv_off, INF, f32), pv.reshape(-1), np.full(8, INF, f32)])
        it["pvmax"] = pvmax
    return it


def stream_out_blank(it):
    n = it["out_off"] + it["n_mels"] * it["ld"] + SLACK
    return np.full(n, CANARY16, np.uint16) if it["f16"] else canary(n).copy()


HISTS = (1, 3, 4, 7, 8, 9, 32, 33, 50)
_STREAM_TABLES = []


def stream_tables():
    """[(name, [items])]: every table is one call of the entry (at most 64 items, 32 per launch)"""
    if _STREAM_TABLES:
        return _STREAM_TABLES
    tabs, items, i = [], [], 0

    def flush(name):
        while items:
            tabs.append((f"{name}_{len(tabs)}", items[:64]))
            del items[:64]

    for hist in HISTS:                              # histories x frame counts x provisional frames
        for J in (0, 1, hist - 1, hist, hist + 1, 2 * hist + 3, 2 ** 32 + 5):
            for pv in (None, 0, 1, 5, "ld", "above"):
                pv_ld = (6, 9, 13)[i % 3]
                n_new = None if pv is None else pv_ld if pv == "ld" else pv_ld + 4 if pv == "above" else pv
                most = min(J, hist) + (0 if n_new is None else min(n_new, pv_ld))
                if n_new is None and most < 1:
                    continue
                n_frames = max((1, most, most + 2, (most + 1) // 2)[i % 4] if n_new is not None else (most, 1, (most + 1) // 2, most)[i % 4], 1)
                items.append(stream_item(f"sweep_h{hist}_J{J}_pv{pv}_n{n_frames}", hist, J, n_frames, n_frames + i % 3, i & 1, (5, 8, 9)[i % 3], n_new,
                                         pv_ld, i % 4, (i // 4) % 4, (i // 2) % 8, i % 4, 1000 + i, (1.5, -2.25, 0.0)[i % 3]))
                i += 1
    flush("sweep")
    for ring_off in range(4):                       # every source alignment x destination head x dtype, in full
        for pv_off in range(4):
            for out_off in range(8):
                for f16 in (0, 1):
                    J = 40 + i % 33                 # (the wrap and the seam move through the groups as well)
                    items.append(stream_item(f"align_r{ring_off}_p{pv_off}_o{out_off}_f16{f16}_J{J}", 33, J, 31, 31 + i % 2, f16, 5, 3 + i % 9, 11,
                                             ring_off, pv_off, out_off, i % 4, 2000 + i))
                    i += 1
    flush("align")
    for f16 in (0, 1):                              # the wrap at every position of a group; the seam likewise; wholly provisional
        for J in range(33, 49):
            items.append(stream_item(f"wrap_J{J}_f16{f16}", 32, J, 24, 24, f16, 5, None, 0, J % 4, 0, (J // 4) % 8, 0, 3000 + J))
        for n_new in range(1, 17):
            items.append(stream_item(f"seam_P{n_new}_f16{f16}", 32, 45, 28, 28, f16, 5, n_new, 19, n_new % 4, (n_new // 4) % 4, n_new % 8, 1, 3100 + n_new))
        for J, n_frames in ((0, 12), (0, 5), (7, 9), (2 ** 32 + 5, 10)):
            items.append(stream_item(f"provisional_J{J}_n{n_frames}_f16{f16}", 8, J, n_frames, 17, f16, 8, 12, 14, 1, 2, 3, 0, 3200 + n_frames))
    flush("geometry")
    for width in list(range(1, 18)) + [3000]:       # widths; the fill behind the frames
        for f16 in (0, 1):
            n = min(width, 11)
            items.append(stream_item(f"width{width}_f16{f16}", 9, 30, max(n - 2, 1), width, f16, 5, 4, 7, width % 4, width % 3, width % 8, width % 4, 4000 + width))
    flush("width")
    items.extend(tie_items())
    flush("ties")
    base = [stream_item(f"table_{j}", (7, 33, 50)[j % 3], 60 + j, min(5 + j % 12, (7, 33, 50)[j % 3]), 17, j & 1, (5, 80, 8, 128, 9)[j % 5] if j in (1, 3) else (5, 8, 9)[j % 3],
                        None if j % 3 == 0 else j % 7, 8, j % 4, (j + 1) % 4, j % 8, j % 3, 5000 + j) for j in range(22)]
    tabs.append(("table_33", [base[j % 22] for j in range(33)]))          # (items 22 .. 32 repeat the first ones)
    tabs.append(("table_64", [base[(5 * j) % 22] for j in range(64)]))
    _STREAM_TABLES.extend(tabs)
    return tabs


def tie_items():
    out = []
    for f16 in (0, 1):
        it = stream_item(f"ties_f16{f16}", 16, 20, 12, 16, f16, 5, 4, 6, 1, 2, 3, 0, 77, 8.0)
        a, used, n_prov, p0, P = span(it)
        ring = it["ring"][1:1 + 5 * 16].reshape(5, 16)
        for col, v in enumerate((2.0 ** -9, 3 * 2.0 ** -9, 5 * 2.0 ** -9, 0.0)):
            ring[:, (a + col) % 16] = v
            it["fmax"][(a + col) % 16] = v
        ring[2, (a + 4) % 16], it["fmax"][(a + 4) % 16] = 8.0, 8.0
        pv = it["pv"][2:2 + 5 * 6].reshape(5, 6)
        pv[:, p0:P] = 0.0
        pv[1, p0], pv[1, p0 + 1] = 2.0 ** -9, 3 * 2.0 ** -9
        it["pvmax"][p0:P] = 3 * 2.0 ** -9
        out.append(it)
        out.append(stream_item(f"nan_inside_f16{f16}", 9, 14, 8, 12, f16, 5, 3, 5, 2, 1, 5, 1, 78, 1.5, nan_at=(2, 3)))
        out.append(stream_item(f"nan_provisional_f16{f16}", 9, 14, 8, 12, f16, 5, 3, 5, 2, 1, 5, 1, 79, -2.25, nan_at=(4, 7)))
    return out
