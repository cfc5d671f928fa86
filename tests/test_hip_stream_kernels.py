"""Every launch form of the kernels a live stream runs on every push -- csrc/stream.hip and the streamed part of csrc/handoff.hip --
through the host entries of include/css_mi355_stream_kernels.h, against the exact models of tests/stream_reference.py (DESIGN.md
7b "The stream kernels, launch form by launch form").  Three kinds of assertion per launch:

  ownership  every output allocation and 256 elements of slack behind it start as the canary of its type (0x7FC0BEEF, 0xA5,
             0x5A5A5A5A); the WHOLE allocation is compared with the model's, so everything the launch does not own keeps its bits;
             inputs the model does not read are NaN (mask columns behind the slots, samples of dropped blocks, spectra behind n_new,
             the tail and carry floats nothing stands in) or are toggled between two runs (activity bytes out of the morphology's
             reach, ring bytes of frames that are not gated-final) without a bit of any output changing
  value      bit equality with the model; the mel values inside handoff_reference's bound with the product's terms removed (the
             worst error / bound per n_mels is printed), -10.0f bit for bit where the sum surely lies at the floor; gmax, fmax,
             pvmax and the ring as exact functions of the float32 mel the launch itself wrote
  bits       a job in a table against the job alone; a range in two launches against one; the rounds of every cutting against
             the whole recording's concatenation (handoff_reference), hence against each other; a preview's round against the push's

Coverage, one line per launch function and template instance:
  launch_stream_activity_multi          test_tail: (8, 8), (8, 4), (8, 3), (16, 1), (186, 179) x F 5, 16, 17, 257 x S 1, 3, 4; windows at base
                                        0 and above, open and closing; ranges of 0, 1, 15, 16, 17, 33 frames off the 16-frame grid; the
                                        mean at the threshold and its neighbours; test_tail_tables: 17 and 33 jobs, one empty, the longest last
  launch_stream_gate_ola_multi          test_tail: the same x (dilation, erosion) (0, 0), (3, 1), (5, 0), (0, 5), (2, 130: the staging loop's
                                        second pass) x KIp 2 F, rounded to 32, + 32 x five gate kinds x ring 32, 64 (the wrap inside the
                                        range) and absent; the last block's lanes past the row's end; closing with T_long_global inside
                                        a block; test_tail_split: two launches against one; test_tail_tables: mixed erosions (the launch's
                                        LDS is the largest entry's) and bases
  launch_stream_scatter_masks           test_scatter: rows 1, 3, 4, 5, 1028 x 1, 16, 17, 33 entries x n_cols 0, 1, 63, 64, 65, 186, 372 x
                                        source columns and destination offsets 0 .. 3 mod 4
  launch_stream_ingest_pcm16_multi      test_ingest: C 1, 2, 7, 8, 64 x interleaved, planar, planar with plane_ld > n x n 0, 1, 7, 8, 9, 63,
                                        64, 65, tile - 1, tile, tile + 1, 2 tile + 3 x destination columns 0 .. 3, in tables of 17
  launch_handoff_append_multi           test_append: pad 0, 1, 3, 8, 300 x drop on, off x six gates x cuttings of 1, 7, 16, 100 frames and
                                        all at once; an open and a closing round of more than 256 blocks; closing at 0, 150, 180 and 256
                                        samples; every round as a push and as a preview; test_append_far_state: A, J beyond 2^32;
                                        test_append_table: 17 streams x 3 speakers
  launch_handoff_mel_multi <false>      test_mel[false]: n_mels 80, 128 x n_new 0, 1, 31, 32, 33, rows, above rows x gmax presets x seven
                                        kinds of spectra x histories of 8, 16, 50 frames, J beyond 2^32, in a table of 17
  launch_handoff_mel_multi <true>       test_mel[true]: the same table with pvmax entries among the others
  the entries' refusals                 test_refusals
Needs an MI355X."""
import numpy as np
import pytest

import handoff_reference as H
import stream_reference as R
from conftest import pkg

pytestmark = pytest.mark.gpu

SLACK = 256                  # elements of slack behind every output


def _open():
    L = pkg("_lib")
    if L.load().css_device_count() < 1:
        pytest.fail("no HIP device visible")
    w = pkg("weights")
    desc = w.ModelDesc(num_blocks=1)
    return pkg("separator").HipSeparator(w.apply_golden_recipe(w.portable_state_dict(desc, 5)), None, device=0)


@pytest.fixture(scope="module")
def handle():
    sep = _open()
    yield sep.handle
    sep.close()


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.size == 0:
        return
    ua, ub = a.view(np.uint8).reshape(a.size, -1), b.view(np.uint8).reshape(b.size, -1)
    diff = np.flatnonzero((ua != ub).any(axis=-1))
    assert diff.size == 0, (what, f"{len(diff)} of {a.size} values differ, the first at {diff[0]}: {a[diff[0]]!r} != {b[diff[0]]!r}")


def _with_slack(a, fill):
    """the array flattened, with SLACK canaries behind it"""
    a = np.ascontiguousarray(a).reshape(-1)
    return np.concatenate([a, np.full(SLACK, fill, a.dtype)])


# ---- the stitching tail -------------------------------------------------------------------------------------------------------------

def _tail_job(w, a, lo, hi, act_b, Y, ring):
    job = dict(w, t_lo=lo, t_hi=hi, masks=a["masks"], sep=a["sep"], perms=a["perms"], w_first=a["w_first"], w_mid=a["w_mid"], w_last=a["w_last"],
               act_b=_with_slack(act_b, R.CANARY_BYTE))
    job["Y"] = np.concatenate([R.bits(Y).reshape(-1), np.full(SLACK, R.CANARY, np.uint32)]).view(np.float32)
    if ring is not None:
        job["ring"] = _with_slack(ring, R.CANARY_BYTE)
    else:
        job["gate_ld"] = 0
    return job


def _blank(w):
    S, ld = w["S"], w["ld_frames"]
    return (R.canary8(S * ld).reshape(S, ld), R.canary(S * ld * w["KIp"]).reshape(S, ld, w["KIp"]), R.canary8(S * w["gate_ld"]).reshape(S, -1))


def _toggled(w, act, lo, hi, value):
    """act_b with everything out of the morphology's reach of [lo, hi) set to `value`"""
    r_lo, r_hi = R.morph_reads(w, lo, hi)
    out = np.full_like(act, value)
    if hi > lo:
        out[:, max(r_lo, 0):r_hi] = act[:, max(r_lo, 0):r_hi]
    return out


def _check_tail_job(handle, w, a, lo, hi, with_ring, what):
    S, ld, KIp = w["S"], w["ld_frames"], w["KIp"]
    win = (a["w_first"], a["w_mid"], a["w_last"])
    act0, Y0, ring0 = _blank(w)
    # form 0: the activity bytes of [lo, hi) and nothing else
    got, = handle.stream_tail(0, [_tail_job(w, a, lo, hi, act0, Y0, ring0 if with_ring else None)])
    want = R.activity(w, a["masks"], win, a["perms"], lo, hi, act0)
    _same_bits(got["act_b"], _with_slack(want, R.CANARY_BYTE), what + ": act_b")
    _same_bits(got["Y"], _tail_job(w, a, lo, hi, act0, Y0, None)["Y"], what + ": form 0 leaves Y alone")
    # form 1 on the case's activity bytes, twice: what lies out of the morphology's reach is 0xA5 once and 0 once
    outs = []
    for value in (R.CANARY_BYTE, 0):
        act = _toggled(w, a["act_b"], lo, hi, value)
        got, = handle.stream_tail(1, [_tail_job(w, a, lo, hi, act, Y0, ring0 if with_ring else None)])
        _same_bits(got["act_b"], _with_slack(act, R.CANARY_BYTE), what + ": form 1 leaves act_b alone")
        outs.append(got)
    wantY, want_ring = R.gate_ola(w, a["sep"], win, a["perms"], a["act_b"], lo, hi, Y0, ring0 if with_ring else None)
    for got in outs:
        _same_bits(R.bits(got["Y"]), np.concatenate([R.bits(wantY).reshape(-1), np.full(SLACK, R.CANARY, np.uint32)]), what + ": Y")
        if with_ring:
            _same_bits(got["ring"], _with_slack(want_ring, R.CANARY_BYTE), what + ": ring")
    return wantY, want_ring


@pytest.mark.parametrize("c", R.tail_cases(), ids=lambda c: c["name"])
def test_tail(handle, c):
    for i, (w, a, lo, hi) in enumerate(R.tail_jobs(c)):
        _check_tail_job(handle, w, a, lo, hi, R.tail_with_ring(i), f"{c['name']} base {w['seg_base']} [{lo}, {hi})")


@pytest.mark.parametrize("c", [c for c in R.tail_cases() if c["F"] <= 17][::2], ids=lambda c: c["name"])
def test_tail_split(handle, c):
    """a range in two launches (cut off the 16-frame grid) against one, both forms"""
    for w, a, lo, hi in R.tail_jobs(c):
        if hi - lo < 3:
            continue
        mid = lo + (hi - lo) // 2 + ((hi - lo) // 2 % 16 == 0)
        act0, Y0, ring0 = _blank(w)
        one0, = handle.stream_tail(0, [_tail_job(w, a, lo, hi, act0, Y0, ring0)])
        one1, = handle.stream_tail(1, [_tail_job(w, a, lo, hi, a["act_b"], Y0, ring0)])
        two0, = handle.stream_tail(0, [_tail_job(w, a, lo, mid, act0, Y0, ring0)])
        two0, = handle.stream_tail(0, [dict(_tail_job(w, a, mid, hi, act0, Y0, ring0), act_b=two0["act_b"])])
        two1, = handle.stream_tail(1, [_tail_job(w, a, lo, mid, a["act_b"], Y0, ring0)])
        two1, = handle.stream_tail(1, [dict(_tail_job(w, a, mid, hi, a["act_b"], Y0, ring0), Y=two1["Y"], ring=two1["ring"])])
        what = f"{c['name']} base {w['seg_base']} [{lo}, {mid}) + [{mid}, {hi})"
        _same_bits(two0["act_b"], one0["act_b"], what + ": act_b")
        _same_bits(R.bits(two1["Y"]), R.bits(one1["Y"]), what + ": Y")
        _same_bits(two1["ring"], one1["ring"], what + ": ring")


@pytest.mark.parametrize("n", (17, 33))
def test_tail_tables(handle, n):
    picked = R.tail_table_jobs(n)
    for form in (0, 1):
        jobs = []
        for i, (w, a, lo, hi) in enumerate(picked):
            act0, Y0, ring0 = _blank(w)
            jobs.append(_tail_job(w, a, lo, hi, act0 if form == 0 else a["act_b"], Y0, ring0 if i % 2 == 0 else None))
        together = handle.stream_tail(form, jobs)
        for i, (job, got) in enumerate(zip(jobs, together)):
            alone, = handle.stream_tail(form, [job])
            for name in got:
                _same_bits(got[name].view(np.uint8), alone[name].view(np.uint8), f"form {form} job {i} of {n}: {name}")
        w, a, lo, hi = picked[3]
        assert hi == lo   # the empty job wrote nothing
        _same_bits(together[3]["Y"].view(np.uint32), jobs[3]["Y"].view(np.uint32), "the empty job's Y")
        _same_bits(together[3]["act_b"], jobs[3]["act_b"], "the empty job's act_b")
        # the longest job, last, against the model
        w, a, lo, hi = picked[-1]
        act0, Y0, ring0 = _blank(w)
        if form == 0:
            want = R.activity(w, a["masks"], (a["w_first"], a["w_mid"], a["w_last"]), a["perms"], lo, hi, act0)
            _same_bits(together[-1]["act_b"], _with_slack(want, R.CANARY_BYTE), "the last job's act_b")
        else:
            wantY, _ = R.gate_ola(w, a["sep"], (a["w_first"], a["w_mid"], a["w_last"]), a["perms"], a["act_b"], lo, hi, Y0, None)
            _same_bits(R.bits(together[-1]["Y"])[:wantY.size], R.bits(wantY).reshape(-1), "the last job's Y")


# ---- scatter and ingest -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,n_entries", R.SCATTER_TABLES)
def test_scatter(handle, rows, n_entries):
    rng = np.random.default_rng(rows)
    src = rng.standard_normal((rows, R.SCATTER_SRC_LD)).astype(np.float32)
    entries = R.scatter_entries(n_entries, rows)
    read = np.zeros(R.SCATTER_SRC_LD, bool)
    for e in entries:
        read[e["src_col"]:e["src_col"] + e["n_cols"]] = True
    src[:, ~read] = np.nan                       # columns no entry names
    jobs = [dict(e, dst=R.canary(e["dst_off"] + (rows - 1) * e["dst_ld"] + e["n_cols"] + SLACK)) for e in entries]
    got = handle.stream_scatter(np.concatenate([src.reshape(-1), np.full(SLACK, np.nan, np.float32)]), R.SCATTER_SRC_LD, rows, jobs)
    for i, (e, job, g) in enumerate(zip(entries, jobs, got)):
        _same_bits(R.bits(g["dst"]), R.bits(R.scatter(src, R.SCATTER_SRC_LD, rows, e, job["dst"])), f"rows {rows} entry {i} of {n_entries}: {e}")
    alone, = handle.stream_scatter(src, R.SCATTER_SRC_LD, rows, [jobs[-1]])
    _same_bits(R.bits(alone["dst"]), R.bits(got[-1]["dst"]), "the last entry alone")


@pytest.mark.parametrize("C_", (1, 2, 7, 8, 64))
def test_ingest(handle, C_):
    cases = [c for c in R.ingest_cases() if c["C"] == C_]
    jobs, wants = [], []
    for c in cases:
        src, plane_ld, dst, dst_ld = R.ingest_inputs(c)
        jobs.append(dict(C=C_, dst_col=c["dst_col"], plane_ld=plane_ld, n=c["n"], dst_ld=dst_ld, src=src, dst=dst))
        wants.append(R.ingest(src, C_, c["n"], plane_ld, dst, c["dst_col"], dst_ld))
    for i0 in range(0, len(jobs), 17):           # tables of 17 (the last one shorter): each crosses the kernel's table of 16
        got = handle.stream_ingest(jobs[i0:i0 + 17])
        for c, g, want in zip(cases[i0:], got, wants[i0:]):
            _same_bits(R.bits(g["dst"]), R.bits(want), c["name"])
    for i in range(0, len(jobs), 5):
        alone, = handle.stream_ingest([jobs[i]])
        _same_bits(R.bits(alone["dst"]), R.bits(wants[i]), cases[i]["name"] + " alone")


# ---- append -----------------------------------------------------------------------------------------------------------------------

def _append_call_job(job, preview):
    """the entry's job of a model job: outputs as canaries with slack"""
    S, nt = job["S"], job["t_g1"] - job["t_g0"]
    out = {k: v for k, v in job.items()}
    out["carry_out"] = R.canary(S * job["carry_ld"] + SLACK)
    out["tail_out"] = R.canary(S * R.TAIL_LD + SLACK)
    out["act_out"] = R.canary8(S * nt + SLACK)
    out["n_new"] = np.full(S + SLACK, R.CANARY32, np.int32)
    if preview:
        out["st_out"] = np.frombuffer(np.full(24 * (S + 8), R.CANARY_BYTE, np.uint8).tobytes(), R.STATE).copy()
    return out


def _check_append_result(job, got, operand, models, preview, what, defs=None):
    S, nt = job["S"], job["t_g1"] - job["t_g0"]
    rows, row0 = got["rows"], got["row0"]
    assert rows == models[0]["rows"], what
    st_after = got["st_out"][:S] if preview else got["st"][:S]
    if preview:
        _same_bits(got["st"].view(np.uint8), np.ascontiguousarray(job["st"]).view(np.uint8), what + ": a preview leaves st alone")
        _same_bits(got["st_out"][S:].view(np.uint8), np.full(24 * 8, R.CANARY_BYTE, np.uint8), what + ": behind st_out")
    carry = got["carry_out"][:S * job["carry_ld"]].reshape(S, -1)
    tail = got["tail_out"][:S * R.TAIL_LD].reshape(S, -1)
    for k, m in enumerate(models):
        w = f"{what} speaker {k}"
        assert (int(st_after[k]["A"]), int(st_after[k]["J"]), int(got["n_new"][k])) == (m["A1"], m["J1"], m["n_new"]), (w, st_after[k], m["A1"], m["J1"])
        assert st_after[k]["gmax"] == job["st"][k]["gmax"], w + ": gmax"
        op = operand[(row0 + k * rows) * 160:(row0 + (k + 1) * rows) * 160]
        _same_bits(R.bits(op[:m["defined"]]), R.bits(m["operand"][:m["defined"]]), w + ": the operand columns the round's frames read")
        assert np.isfinite(op).all(), w + ": an operand column of the speaker's rows is not finite"
        if defs is not None and m["defined"]:
            J0 = int(job["st"][k]["J"])
            seg = defs[k][2][160 * J0:160 * J0 + m["defined"]]
            _same_bits(R.bits(op[:len(seg)]), R.bits(seg), w + ": the operand against the whole recording's")
            assert (op[len(seg):m["defined"]] == 0).all()
        n_t = len(m["tail"])
        _same_bits(R.bits(tail[k, m["tail_at"]:m["tail_at"] + n_t]), R.bits(m["tail"]), w + ": tail_out")
        _same_bits(R.bits(tail[k, :m["tail_at"]]), np.zeros(m["tail_at"], np.uint32), w + ": the floats of tail_out before sample 0")
        assert (R.bits(tail[k, m["tail_at"] + n_t:]) == R.CANARY).all(), w + ": behind the tail"
        _same_bits(R.bits(carry[k, :len(m["carry"])]), R.bits(m["carry"]), w + ": carry_out")
        assert (R.bits(carry[k, len(m["carry"]):]) == R.CANARY).all(), w + ": behind the carry"
        _same_bits(got["act_out"][k * nt:(k + 1) * nt], m["act"], w + ": act_out")
    assert (R.bits(got["carry_out"][S * job["carry_ld"]:]) == R.CANARY).all() and (R.bits(got["tail_out"][S * R.TAIL_LD:]) == R.CANARY).all()
    assert (got["act_out"][S * nt:] == R.CANARY_BYTE).all() and (got["n_new"][S:] == R.CANARY32).all(), what + ": slack"
    return carry, tail, st_after.copy()


def _append_round(handle, c, rnd, state, what, defs=None, also_preview=False):
    """one round on the device, with the ring bytes the round may not look at as 1 and as 0; returns the state it leaves"""
    left = None
    for junk in (1, 0):
        job = R.append_job(c, rnd, state, junk=junk)
        models = [R.append_round(job, k) for k in range(c["S"])]
        n_op = models[0]["rows"] * c["S"] * 160 + 1024
        for preview in ((False, True) if also_preview and junk else (False,)):
            (got,), operand = handle.stream_append([_append_call_job(job, preview)], R.canary(n_op))
            assert (R.bits(operand[n_op - 1024:]) == R.CANARY).all(), what + ": the operand's tail of 1024 floats"
            res = _check_append_result(job, got, operand, models, preview, f"{what} junk {junk} preview {preview}", defs)
            if not preview and left is None:
                left = res
    return left


@pytest.mark.parametrize("c", R.append_cases(), ids=lambda c: c["name"])
def test_append(handle, c):
    defs = [R.append_definition(c, k) for k in range(c["S"])]
    state = R.append_state0(c["S"], c["carry_ld"])
    rounds = R.append_rounds(c)
    for i, rnd in enumerate(rounds):
        state = _append_round(handle, c, rnd, state, f"{c['name']} round {rnd}", defs, also_preview=(i % 3 == 0 or rnd[4] == 1))
    for k in range(c["S"]):
        assert int(state[2][k]["A"]) == len(defs[k][0]) and int(state[2][k]["J"]) == defs[k][1], (c["name"], k)


def test_append_far_state(handle):
    c, state, rounds = R.append_big_state()
    for rnd in rounds:
        state = _append_round(handle, c, rnd, state, f"far state round {rnd}", None, also_preview=True)
    assert all(int(s["A"]) > R.BIG and int(s["J"]) == int(s["A"]) // 160 for s in state[2])


def test_append_table(handle):
    """17 streams x 3 speakers in one call (two launches): every job against the job alone"""
    cases = [c for c in R.append_cases() if c["TL"] < 200][:17]
    assert len(cases) == 17
    jobs, models = [], []
    for i, c in enumerate(cases):
        rounds = R.append_rounds(c)
        state = R.append_state0(c["S"], c["carry_ld"])
        for rnd in rounds[:min(i % 3, len(rounds) - 1)]:     # (the job is the case's first, second or third round)
            job = R.append_job(c, rnd, state)
            state = R.append_next(job, [R.append_round(job, k) for k in range(c["S"])])
        job = R.append_job(c, rounds[min(i % 3, len(rounds) - 1)], state)
        jobs.append(job)
        models.append([R.append_round(job, k) for k in range(c["S"])])
    n_op = sum(m[0]["rows"] * 3 * 160 for m in models) + 1024
    together, operand = handle.stream_append([_append_call_job(j, i % 4 == 1) for i, j in enumerate(jobs)], R.canary(n_op))
    assert (R.bits(operand[n_op - 1024:]) == R.CANARY).all()
    for i, (job, got, m) in enumerate(zip(jobs, together, models)):
        _check_append_result(job, got, operand, m, i % 4 == 1, f"table job {i} ({cases[i]['name']})")
        (alone,), op1 = handle.stream_append([_append_call_job(job, i % 4 == 1)], R.canary(m[0]["rows"] * 3 * 160 + 1024))
        for name in ("carry_out", "tail_out", "act_out", "n_new", "st"):
            _same_bits(got[name].view(np.uint8), alone[name].view(np.uint8), f"table job {i}: {name}")
        own = m[0]["rows"] * 3 * 160
        _same_bits(R.bits(operand[got["row0"] * 160:got["row0"] * 160 + own]), R.bits(op1[:own]), f"table job {i}: operand")


# ---- mel --------------------------------------------------------------------------------------------------------------------------

def _preset(name):
    return {"reset": R.GMAX_NONE, "below": R.order_int(R.f32(-20.0)), "above": R.order_int(R.f32(30.0))}[name]


def _mel_job(c, row0, pv):
    S, nm, rows, hist = 3, c["n_mels"], c["rows"], c["hist"]
    st = np.zeros(S, R.STATE)
    for k in range(S):
        st[k]["A"], st[k]["J"], st[k]["gmax"], st[k]["pad"] = 160 * c["J"][k] + 40, c["J"][k], _preset(c["presets"][k]), 0x5A5A
    job = dict(n_mels=nm, row0=row0, rows=rows, hist=hist, mel_ld=rows + 3, n_new=np.array(c["n_new"], np.int32), st=st,
               mel=R.canary(S * nm * (rows + 3) + SLACK))
    if c["form"] == "ring":
        job["ring"], job["fmax"] = R.canary(S * nm * hist + SLACK), R.canary(S * hist + SLACK)
    if c["form"] == "pvmax" and pv:
        job["pvmax"] = R.canary(S * rows + SLACK)
    return job


@pytest.mark.parametrize("pv", (False, True), ids=("false", "true"))
def test_mel(handle, pv):
    """a table of 17 jobs (two launches); with pv the pvmax cases carry their pvmax array and their launch is the <true> instance"""
    cases = [c for c in R.mel_cases() if pv or c["form"] != "pvmax"]
    picked = [cases[i % len(cases)] for i in range(17)]
    if pv:   # a pvmax entry in both launches of the call
        picked[0], picked[16] = [c for c in cases if c["form"] == "pvmax"]
    row0s = np.concatenate([[2], 2 + np.cumsum([3 * c["rows"] + 1 for c in picked])])
    ld = int(row0s[-1]) + 5
    spec = np.full((402, ld), np.nan, np.float32)
    for c, row0 in zip(picked, row0s):
        R.mel_case_spec(c, int(row0), ld, spec)
    jobs = [_mel_job(c, int(row0), pv) for c, row0 in zip(picked, row0s)]
    got = handle.stream_mel(3, spec, ld, jobs)
    worst = {80: (0.0, "-"), 128: (0.0, "-")}
    for i, (c, job, g) in enumerate(zip(picked, jobs, got)):
        nm, rows, mel_ld, hist = c["n_mels"], c["rows"], job["mel_ld"], c["hist"]
        mel = g["mel"][:3 * nm * mel_ld].reshape(3, nm, mel_ld)
        assert (R.bits(g["mel"][3 * nm * mel_ld:]) == R.CANARY).all()
        for k in range(3):
            what = f"job {i} ({c['name']}) speaker {k}"
            nfr = min(c["n_new"][k], rows)
            assert (R.bits(mel[k, :, nfr:]) == R.CANARY).all(), what + ": mel behind n_new"
            if nfr:
                raw, e_raw, floor = R.mel_reference(spec, ld, int(job["row0"]) + k * rows, nfr, nm)
                v = mel[k, :, :nfr]
                assert (R.bits(v[floor]) == R.bits(np.array([H.LOG_FLOOR]))[0]).all(), what + ": -10.0f at the floor"
                err = np.abs(v.astype(np.float64) - raw)
                ratio = np.where(floor | (err == 0), 0.0, err / np.maximum(e_raw, 1e-300))
                pos = np.unravel_index(int(ratio.argmax()), ratio.shape)
                assert ratio[pos] <= 1.0, (what, f"error / bound {ratio[pos]:.3f} at {pos}: {v[pos]!r} against {raw[pos]!r}, bound {e_raw[pos]!r}")
                if ratio[pos] > worst[nm][0]:
                    worst[nm] = (float(ratio[pos]), what)
            gmax, fm, slots = R.mel_side(mel[k], c["n_new"][k], rows, c["J"][k], job["st"][k]["gmax"], hist if c["form"] == "ring" else 0)
            assert g["st"][k]["gmax"] == gmax, (what, "gmax", g["st"][k]["gmax"], gmax)
            assert (g["st"][k]["A"], g["st"][k]["J"], g["st"][k]["pad"]) == (job["st"][k]["A"], job["st"][k]["J"], 0x5A5A), what
            if c["form"] == "ring":
                ring = g["ring"][:3 * nm * hist].reshape(3, nm, hist)
                fmax = g["fmax"][:3 * hist].reshape(3, hist)
                want_r, want_f = R.canary(nm * hist).reshape(nm, hist), R.canary(hist)
                for slot, j in slots.items():
                    want_r[:, slot], want_f[slot] = mel[k, :, j], fm[j]
                _same_bits(R.bits(ring[k]), R.bits(want_r), what + ": ring")
                _same_bits(R.bits(fmax[k]), R.bits(want_f), what + ": fmax")
            if "pvmax" in job:
                want_p = R.canary(rows)
                want_p[:nfr] = fm
                _same_bits(R.bits(g["pvmax"][k * rows:(k + 1) * rows]), R.bits(want_p), what + ": pvmax")
        for name in ("ring", "fmax", "pvmax"):
            if name in g:
                assert (R.bits(g[name][-SLACK:]) == R.CANARY).all(), f"job {i}: behind {name}"
    print("\n" + "\n".join(f"  worst error / bound of the mel values, n_mels {nm}: {r:.3f} [{w}]" for nm, (r, w) in worst.items()))
    for i in (0, 5, 16):                         # a job in the table against the job alone
        alone, = handle.stream_mel(3, spec, ld, [jobs[i]])
        for name in got[i]:
            _same_bits(got[i][name].view(np.uint8), alone[name].view(np.uint8), f"job {i} alone: {name}")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def _refused(call, jobs, what, *args):
    L = pkg("_lib")
    before = [{k: v.copy() for k, v in j.items() if isinstance(v, np.ndarray)} for j in jobs]
    with pytest.raises(L.CssError) as e:
        call(jobs, *args)
    assert "css_stream_" in str(e.value), (what, str(e.value))
    left = e.value.left[0] if isinstance(e.value.left, tuple) else e.value.left
    for j, b, l in zip(jobs, before, left):
        for k, v in b.items():
            _same_bits(j[k].view(np.uint8), v.view(np.uint8), what + ": the caller's " + k)
            if k in l:
                _same_bits(l[k].view(np.uint8), v.reshape(-1).view(np.uint8), what + ": " + k + " as the call left it")


def test_refusals(handle):
    # ---- the tail
    c = R.tail_cases()[1]
    w, a, lo, hi = [j for j in R.tail_jobs(c) if j[0]["seg_base"] > 0 and j[3] - j[2] > 4][0]

    def tail(**kw):
        act0, Y0, ring0 = _blank(w)
        j = _tail_job(w, a, lo, hi, a["act_b"], Y0, ring0)
        j.update(kw)
        return [j]
    for form in (0, 1):
        handle.stream_tail(form, tail())       # (the unchanged job is accepted)
    halo = w["erosion"] + w["dilation"]
    bad = [dict(S=0), dict(S=5), dict(hop=0), dict(hop=w["T"] + 1), dict(KIp=2 * w["F"] - 1), dict(gate_ld=48), dict(t_lo=-1), dict(t_hi=lo - 1),
           dict(t_hi=w["ld_frames"] + 1), dict(num_slots=w["num_slots"] + 1), dict(num_segments_global=w["seg_base"] + w["num_slots"] - 1),
           dict(dilation=-1), dict(erosion=4097), dict(frame_base=-1), dict(F=0), dict(F=1025), dict(T=0), dict(T=4097), dict(seg_base=-1),
           dict(num_slots=-1), dict(masks=a["masks"].reshape(-1)[:w["S"] * w["F"] * w["mask_ld"] - 1]),
           dict(sep=a["sep"].reshape(-1)[:-1]), dict(w_mid=a["w_mid"][:-1]), dict(perms=np.where(a["perms"] == 0, w["S"], a["perms"]))]
    for kw in bad:
        for form in (0, 1):
            _refused(lambda jobs, form=form: handle.stream_tail(form, jobs), tail(**kw), f"tail form {form}: {sorted(kw)}")
    # what form 1 alone reads: the left halo below local frame 0, the block-rounded right reach, the recording's end
    _refused(lambda jobs: handle.stream_tail(1, jobs), tail(t_lo=halo - 1, t_hi=halo + 15), "tail: the left halo")
    handle.stream_tail(0, tail(t_lo=halo - 1, t_hi=halo + 15))
    handle.stream_tail(1, tail(t_lo=halo - 1, t_hi=halo + 15, frame_base=0))
    short = hi - 1 + halo                        # one frame less than the gate of the range's last frame reads
    if short >= hi:
        Ys = R.canary(w["S"] * short * w["KIp"])
        _refused(lambda jobs: handle.stream_tail(1, jobs), tail(ld_frames=short, act_b=a["act_b"][:, :short].copy(), Y=Ys), "tail: the right reach")
        handle.stream_tail(1, tail(ld_frames=short + 1, act_b=a["act_b"][:, :short + 1].copy(), Y=R.canary(w["S"] * (short + 1) * w["KIp"])))
    _refused(lambda jobs: handle.stream_tail(1, jobs), tail(T_long_global=w["frame_base"] + hi - 1, num_segments_global=c["N"]), "tail: past T_long_global")
    for form in (0, 1):
        _refused(lambda jobs, form=form: handle.stream_tail(form, jobs), tail() + tail(S=w["S"] - 1), f"tail form {form}: jobs with different S")
        _refused(lambda jobs, form=form: handle.stream_tail(form, jobs), tail() + tail(F=w["F"] - 1), f"tail form {form}: jobs with different F")
    # the gate launch's LDS: 64 (2 F + 1) + 16 + 2 erosion bytes against 64 KiB (F 511 fits without erosion, not with 130)
    _refused(lambda jobs: handle.stream_tail(1, jobs), tail(F=512), "tail: the LDS at F 512")
    _refused(lambda jobs: handle.stream_tail(1, jobs), tail(F=511, erosion=130), "tail: the LDS at F 511, erosion 130")
    _refused(lambda jobs: handle.stream_tail(2, jobs), tail(), "tail: form 2")
    _refused(lambda jobs: handle.stream_tail(0, jobs), tail() * 65, "tail: 65 jobs")
    # ---- scatter
    src = np.arange(5 * 40, dtype=np.float32)
    sc = lambda **kw: [dict(dict(dst_off=1, dst_ld=12, src_col=3, n_cols=10, dst=R.canary(1 + 4 * 12 + 10)), **kw)]
    handle.stream_scatter(src, 40, 5, sc())
    for kw in (dict(src_col=-1), dict(n_cols=-1), dict(src_col=31), dict(dst_ld=9), dict(dst_off=64), dict(dst_off=-1), dict(dst=R.canary(1 + 4 * 12 + 9))):
        _refused(lambda jobs: handle.stream_scatter(src, 40, 5, jobs), sc(**kw), f"scatter: {sorted(kw)}")
    _refused(lambda jobs: handle.stream_scatter(src, 40, 0, jobs), sc(), "scatter: rows 0")
    _refused(lambda jobs: handle.stream_scatter(src, 40, 6, jobs), sc(), "scatter: src shorter than rows")
    _refused(lambda jobs: handle.stream_scatter(src, 40, 5, jobs), sc() * 65, "scatter: 65 jobs")
    # ---- ingest
    ing = lambda **kw: [dict(dict(C=7, dst_col=2, plane_ld=0, n=9, dst_ld=12, src=np.arange(63, dtype=np.int16), dst=R.canary(2 + 6 * 12 + 9)), **kw)]
    handle.stream_ingest(ing())
    for kw in (dict(C=0), dict(C=65), dict(n=-1), dict(n=(1 << 24) + 1), dict(plane_ld=8), dict(plane_ld=-1), dict(dst_col=4), dict(dst_col=-1),
               dict(dst_ld=10), dict(src=np.arange(62, dtype=np.int16)), dict(dst=R.canary(2 + 6 * 12 + 8)), dict(plane_ld=10)):
        _refused(handle.stream_ingest, ing(**kw), f"ingest: {sorted(kw)} {kw.get('plane_ld')}")
    _refused(handle.stream_ingest, ing() + ing(C=1), "ingest: jobs with different C")
    _refused(handle.stream_ingest, ing() * 65, "ingest: 65 jobs")
    # ---- append
    ca = [c for c in R.append_cases() if c["name"] == "pad3_pauses_16"][0]
    rounds = R.append_rounds(ca)
    state = R.append_state0(ca["S"], ca["carry_ld"])
    job0 = R.append_job(ca, rounds[0], state)
    state = R.append_next(job0, [R.append_round(job0, k) for k in range(3)])
    job1 = R.append_job(ca, rounds[1], state)
    n_op = R.handoff_rows(job1["D1"] - job1["D0"]) * 3 * 160 + 1024

    def app(**kw):
        j = _append_call_job(job1, kw.pop("preview", False))
        j.update(kw)
        return [j]
    call = lambda jobs, n=n_op: handle.stream_append(jobs, R.canary(n))
    call(app())
    call(app(preview=True))
    st_bad = job1["st"].copy()
    st_bad[1]["J"] += 1
    st_neg = job1["st"].copy()
    st_neg[0]["A"] = -1
    bad = [dict(S=0), dict(S=5), dict(pad=-1), dict(pad=4097), dict(gate_ld=48), dict(t_g1=job1["t_g0"] - 1), dict(D1=job1["D0"] - 256), dict(D0=job1["D0"] + 1),
           dict(out_base=-1), dict(out_ld=job1["out_ld"] - 1), dict(carry_ld=job1["out_base"] - job1["D0"] - 1), dict(D1=job1["D1"] + 256),
           dict(gate_ld=8, gate=job1["gate"][:, :8].copy()), dict(st=st_bad), dict(st=st_neg), dict(st=job1["st"][:2]), dict(gate=job1["gate"][:2]),
           dict(tail_in=job1["tail_in"][:, :-1]), dict(n_new=np.zeros(2, np.int32)), dict(act_out=R.canary8(3 * (job1["t_g1"] - job1["t_g0"]) - 1)),
           dict(drop=2), dict(closing=-1), dict(t_g0=-1), dict(D0=-256), dict(D1=job1["D0"] + (1 << 24) + 256),
           dict(D1=job1["D1"] - 256)]      # (the last: 256 t_g1 - D1 > carry_ld alone; out_base - D0 still fits)
    assert job1["out_base"] - job1["D0"] <= job1["carry_ld"] < 256 * job1["t_g1"] - (job1["D1"] - 256) and job1["D1"] - 256 >= job1["D0"]
    for kw in bad:
        _refused(call, app(**kw), f"append: {sorted(kw)}")
    _refused(lambda jobs: call(jobs, n_op - 1), app(), "append: operand one float short")
    _refused(lambda jobs: call(jobs, n_op + 1), app(), "append: operand one float long")
    _refused(lambda jobs: call(jobs, 2 * n_op - 1024), app() + app(S=2), "append: jobs with different S")
    # ---- mel
    cm = R.mel_cases()[4]
    ld = 2 + 3 * cm["rows"] + 4
    spec = np.zeros((402, ld), np.float32)
    mel = lambda **kw: [dict(_mel_job(cm, 2, False), **kw)]
    mcall = lambda jobs, S=3, ld=ld: handle.stream_mel(S, spec, ld, jobs)
    mcall(mel())
    st_low = _mel_job(cm, 2, False)["st"]
    st_low[0]["J"] = cm["n_new"][0] - 1
    for kw in (dict(n_mels=64), dict(row0=-1), dict(rows=0), dict(row0=7), dict(mel_ld=cm["rows"] - 1), dict(n_new=np.array([1, -1, 2], np.int32)),
               dict(hist=0), dict(st=st_low), dict(fmax=R.canary(3 * cm["hist"] - 1)), dict(mel=R.canary(10)), dict(pvmax=R.canary(3 * cm["rows"]))):
        _refused(mcall, mel(**kw), f"mel: {sorted(kw)}")
    _refused(lambda jobs: mcall(jobs, S=0), mel(), "mel: S 0")
    _refused(lambda jobs: mcall(jobs, S=5), mel(), "mel: S 5")
    _refused(lambda jobs: mcall(jobs, ld=ld + 1), mel(), "mel: spec shorter than [402][ld]")
    _refused(mcall, mel() * 65, "mel: 65 jobs")
