"""The two kernels of a round of the streamed NeMo hand-off on caller data (include/css_mi355_stream_nemo.h:
css_stream_nemo_append_host, css_stream_nemo_mel_host; csrc/nemo_stream.hip), on the MI355X.

  launch_nemo_append_multi   test_append: every round of a case against tests/stream_nemo_reference.py's model of it, bit for bit --
                             the speaker's WHOLE operand rows (every float of them is defined), the tail, the carry, the gate bytes,
                             the counts, the last kept sample -- with the ring bytes the round may not look at as 1 and as 0;
                             p = 0.97 and p = 0; seams on round boundaries, rounds that append nothing, A crossing 256, A < 160,
                             160 <= A < 256, a speaker never active (a closing round with A1 = 0), pads 0 .. 300, an open and a
                             closing round of more than 256 blocks (the compaction loop's second pass)
                             test_append_tables: tables of 1, 17 and 33 jobs, every job against the job alone
                             test_append_alone_and_in_the_middle: a speaker alone against the same speaker as the middle one of three
  launch_nemo_mel_multi      test_mel: n_mels 80, 128 x n_new 0, 1, 31, 32, 33, rows, above rows in tables of 1, 17 and 33 jobs: within
                             the counted bound of the float64 value of the same spectra (tests/nemo_reference.py bound with an exact
                             product), no element left out; every job against the job alone; a speaker alone against the middle one
  the entries' refusals      test_refusals: every refusal, with every array as it was
Ownership: every output allocation and 256 elements of slack behind it start as the canary of its type, and every element a launch
does not own must still hold it.  Needs an MI355X."""
import numpy as np
import pytest

import nemo_reference as N
import stream_nemo_reference as M
import stream_reference as R
from conftest import pkg

pytestmark = pytest.mark.gpu

SLACK = 256
APPEND_CASES = [c for c in M.cases() if c["cut"] == "explicit" or c["name"] in (
    "pad0_pauses_every_frame", "pad1_silent_7", "pad3_all_active_16", "pad8_pauses_7", "nodrop_pad8_pauses_every_frame", "pad300_closing_pass2",
    "open_pass2", "closing_150", "closing_180", "closing_256")]


@pytest.fixture(scope="module")
def handle():
    L = pkg("_lib")
    if L.load().css_device_count() < 1:
        pytest.fail("no HIP device visible")
    w = pkg("weights")
    sep = pkg("separator").HipSeparator(w.apply_golden_recipe(w.portable_state_dict(w.ModelDesc(num_blocks=1), 5)), None, device=0)
    yield sep.handle
    sep.close()


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.size and not np.array_equal(a, b):
        i = int(np.flatnonzero(a != b)[0])
        raise AssertionError(f"{what}: {int((a != b).sum())} of {a.size} differ, first at {i}: {a[i]} != {b[i]}")


# ---- append -----------------------------------------------------------------------------------------------------------------------

def _call_job(job):
    """the entry's job of a model job: outputs as canaries with slack"""
    S, nt = job["S"], job["t_g1"] - job["t_g0"]
    out = dict(job)
    out["carry_out"] = R.canary(S * job["carry_ld"] + SLACK)
    out["tail_out"] = R.canary(S * M.TAIL_LD + SLACK)
    out["act_out"] = R.canary8(S * nt + SLACK)
    out["n_new"] = np.full(S + SLACK, R.CANARY32, np.int32)
    out["xlast_out"] = R.canary(S + SLACK)
    return out


def _check(job, got, operand, models, what):
    S, nt = job["S"], job["t_g1"] - job["t_g0"]
    rows, row0 = got["rows"], got["row0"]
    assert rows == models[0]["rows"] == M.nemo_rows(job["D1"] - job["D0"]), what
    st = got["st"][:S]
    carry = got["carry_out"][:S * job["carry_ld"]].reshape(S, -1)
    tail = got["tail_out"][:S * M.TAIL_LD].reshape(S, -1)
    for k, m in enumerate(models):
        w = f"{what} speaker {k}"
        assert (int(st[k]["A"]), int(st[k]["J"]), int(got["n_new"][k])) == (m["A1"], m["J1"], m["n_new"]), (w, st[k], m["A1"], m["J1"])
        assert st[k]["gmax"] == job["st"][k]["gmax"] and st[k]["pad"] == job["st"][k]["pad"], w + ": the state row's other words"
        op = operand[(row0 + k * rows) * 160:(row0 + (k + 1) * rows) * 160]
        _same_bits(M.bits(op), M.bits(m["operand"]), w + ": the speaker's operand rows, all of them")
        n_t = len(m["tail"])
        _same_bits(M.bits(tail[k, :n_t]), M.bits(m["tail"]), w + ": tail_out")
        assert (M.bits(tail[k, n_t:]) == R.CANARY).all(), w + ": behind the tail"
        _same_bits(M.bits(carry[k, :len(m["carry"])]), M.bits(m["carry"]), w + ": carry_out")
        assert (M.bits(carry[k, len(m["carry"]):]) == R.CANARY).all(), w + ": behind the carry"
        _same_bits(got["act_out"][k * nt:(k + 1) * nt], m["act"], w + ": act_out")
        _same_bits(M.bits(got["xlast_out"][k:k + 1]), M.bits(np.array([m["xlast"]], np.float32)), w + ": xlast_out")
    assert (M.bits(got["carry_out"][S * job["carry_ld"]:]) == R.CANARY).all() and (M.bits(got["tail_out"][S * M.TAIL_LD:]) == R.CANARY).all()
    assert (got["act_out"][S * nt:] == R.CANARY_BYTE).all() and (got["n_new"][S:] == R.CANARY32).all(), what + ": slack"
    assert (M.bits(got["xlast_out"][S:]) == R.CANARY).all(), what + ": behind xlast_out"


@pytest.mark.parametrize("c", APPEND_CASES, ids=lambda c: c["name"])
def test_append(handle, c):
    state = M.state0(c)
    rounds = M.rounds_of(c)
    for i, rnd in enumerate(rounds):
        # (the ring bytes the round may not look at as 1, and -- on every fourth round and the closing one -- as 0 as well)
        for junk in ((1, 0) if i % 4 == 0 or rnd[4] else (1,)):
            job = M.job_of(c, rnd, state, junk=junk)
            models = [M.append_round(job, k) for k in range(c["S"])]
            n_op = models[0]["rows"] * c["S"] * 160 + 1024
            (got,), operand = handle.stream_nemo_append([_call_job(job)], R.canary(n_op))
            assert (M.bits(operand[n_op - 1024:]) == R.CANARY).all(), "the operand's tail of 1024 floats"
            _check(job, got, operand, models, f"{c['name']} round {rnd} junk {junk}")
        state = M.next_state(job, models)
    for k in range(c["S"]):
        _, fr, x = M.definition(c, k)
        assert int(state[2][k]["A"]) == len(x) and int(state[2][k]["J"]) == len(fr), (c["name"], k)
    if c["name"] == "seam_on_round_boundary":
        assert int(state[2][1]["A"]) == 0    # (its closing round: A1 = 0)


def _table_jobs(n):
    """n jobs, each the first, second or third round of a case (cases of few frames, cycled), with their models"""
    cases = [c for c in M.cases() if c["TL"] < 100]
    jobs, models = [], []
    for i in range(n):
        c = cases[i % len(cases)]
        rounds = M.rounds_of(c)
        state = M.state0(c)
        stop = min((i // len(cases) + i) % 3, len(rounds) - 1)
        for rnd in rounds[:stop]:
            job = M.job_of(c, rnd, state)
            state = M.next_state(job, [M.append_round(job, k) for k in range(c["S"])])
        job = M.job_of(c, rounds[stop], state)
        jobs.append(job)
        models.append([M.append_round(job, k) for k in range(c["S"])])
    return jobs, models


@pytest.mark.parametrize("n", (1, 17, 33))
def test_append_tables(handle, n):
    """n streams x 3 speakers in one call (tables of 16: one, two and three launches): every job against its model and against the
    job alone"""
    jobs, models = _table_jobs(n)
    n_op = sum(m[0]["rows"] * 3 * 160 for m in models) + 1024
    together, operand = handle.stream_nemo_append([_call_job(j) for j in jobs], R.canary(n_op))
    assert (M.bits(operand[n_op - 1024:]) == R.CANARY).all()
    for i, (job, got, m) in enumerate(zip(jobs, together, models)):
        _check(job, got, operand, m, f"table of {n}, job {i}")
        own = m[0]["rows"] * 3 * 160
        (alone,), op1 = handle.stream_nemo_append([_call_job(job)], R.canary(own + 1024))
        for name in ("carry_out", "tail_out", "act_out", "n_new", "st", "xlast_out"):
            _same_bits(got[name].view(np.uint8), alone[name].view(np.uint8), f"table of {n}, job {i}: {name}")
        _same_bits(M.bits(operand[got["row0"] * 160:got["row0"] * 160 + own]), M.bits(op1[:own]), f"table of {n}, job {i}: operand")


def test_append_alone_and_in_the_middle(handle):
    """speaker 1 of a job of three as a job of one: the same bits in everything that is the speaker's"""
    c = next(c for c in M.cases() if c["name"] == "pad3_seams")
    c = dict(c)
    wav, gate = c["_rec"]
    c["_rec"] = (wav, gate[[1, 0, 2]])          # (the speaker with three ranges in the middle)
    state = M.state0(c)
    for rnd in M.rounds_of(c):
        job = M.job_of(c, rnd, state)
        models = [M.append_round(job, k) for k in range(3)]
        (three,), op3 = handle.stream_nemo_append([_call_job(job)], R.canary(models[0]["rows"] * 3 * 160 + 1024))
        one = dict(job, S=1, **{name: job[name][1:2].copy() for name in ("gate", "out", "carry_in", "tail_in", "st", "xlast_in")})
        (single,), op1 = handle.stream_nemo_append([_call_job(one)], R.canary(models[0]["rows"] * 160 + 1024))
        _check(one, single, op1, models[1:2], f"alone, round {rnd}")
        rows, nt = three["rows"], rnd[1] - rnd[0]
        _same_bits(M.bits(op3[rows * 160:2 * rows * 160]), M.bits(op1[:rows * 160]), "operand")
        _same_bits(M.bits(three["tail_out"][M.TAIL_LD:2 * M.TAIL_LD]), M.bits(single["tail_out"][:M.TAIL_LD]), "tail_out")
        _same_bits(M.bits(three["carry_out"][c["carry_ld"]:2 * c["carry_ld"]]), M.bits(single["carry_out"][:c["carry_ld"]]), "carry_out")
        _same_bits(three["act_out"][nt:2 * nt], single["act_out"][:nt], "act_out")
        assert three["st"][1].tobytes() == single["st"][0].tobytes() and three["n_new"][1] == single["n_new"][0]
        state = M.next_state(job, models)
    assert int(state[2][1]["A"]) > 0


# ---- mel --------------------------------------------------------------------------------------------------------------------------

def _spectra(ld, seed):
    """[514][ld] float32: per column a level between 1e-6 and 10 (quiet columns reach the guard), rows of mixed sign"""
    rng = np.random.default_rng(seed)
    level = 10.0 ** rng.uniform(-6, 1, ld)
    spec = (rng.standard_normal((514, ld)) * level[None, :]).astype(np.float32)
    spec[:, ::7] = 0                                   # digital silence: ln(2^-24)
    return spec


def _mel_reference(spec, col0, nfr, n_mels):
    """float64 values and the counted bound (tests/nemo_reference.py; the spectra are inputs: no rounding of the product)"""
    r = N.Ref()
    _, W = N.tables(n_mels)
    r.W = W
    r.re, r.im = spec[:257, col0:col0 + nfr].astype(np.float64), spec[257:, col0:col0 + nfr].astype(np.float64)
    r.s_re, r.s_im = np.zeros_like(r.re), np.zeros_like(r.im)
    r.power = r.re * r.re + r.im * r.im
    r.mel = W @ r.power
    r.raw = r.out = np.log(r.mel + N.GUARD)
    return r.raw, N.bound(r, normalize=False, k_prod=0)


def _mel_jobs(n, S, ld_out=False):
    """n jobs: n_mels alternates, rows 40 or 70, n_new per speaker from the edge list (rotating); -> (jobs, ld)"""
    edges = (0, 1, 31, 32, 33, None, 1000)              # None: rows itself
    jobs, row0 = [], 3
    for i in range(n):
        rows = 40 if i % 2 else 70
        nn = np.array([rows if edges[(i + k) % 7] is None else edges[(i + k) % 7] for k in range(S)], np.int32)
        nm = 128 if i % 3 == 1 else 80
        jobs.append(dict(n_mels=nm, row0=row0, rows=rows, mel_ld=rows + 3, n_new=nn, mel=R.canary(S * nm * (rows + 3) + SLACK)))
        row0 += S * rows + (i % 2)
    return jobs, row0 + 5


@pytest.mark.parametrize("n", (1, 17, 33))
def test_mel(handle, n):
    S = 3
    jobs, ld = _mel_jobs(n, S)
    spec = _spectra(ld, 40 + n)
    together = handle.stream_nemo_mel(S, spec, ld, jobs)
    worst = 0.0
    for i, (job, got) in enumerate(zip(jobs, together)):
        nm, rows, mel_ld = job["n_mels"], job["rows"], job["mel_ld"]
        mel = got["mel"][:S * nm * mel_ld].reshape(S, nm, mel_ld)
        assert (M.bits(got["mel"][S * nm * mel_ld:]) == R.CANARY).all(), f"job {i}: slack"
        for k in range(S):
            nfr = min(int(job["n_new"][k]), rows)
            assert (M.bits(mel[k, :, nfr:]) == R.CANARY).all(), f"job {i} speaker {k}: behind the frames"
            if nfr == 0:
                continue
            want, bound = _mel_reference(spec, job["row0"] + k * rows, nfr, nm)
            err = np.abs(mel[k, :, :nfr].astype(np.float64) - want)
            assert np.isfinite(mel[k, :, :nfr]).all() and (err <= bound).all(), (i, k, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
        (alone,) = handle.stream_nemo_mel(S, spec, ld, [dict(job, mel=R.canary(job["mel"].size))])
        _same_bits(M.bits(got["mel"]), M.bits(alone["mel"]), f"table of {n}, job {i} against the job alone")
    print(f"table of {n}: largest error / bound {worst:.3f}")
    # a speaker alone (S = 1 on the middle speaker's columns) against the same speaker as the middle one of three
    job = jobs[0]
    nm, rows, mel_ld = job["n_mels"], job["rows"], job["mel_ld"]
    one = dict(job, row0=job["row0"] + rows, n_new=job["n_new"][1:2].copy(), mel=R.canary(nm * mel_ld + SLACK))
    (single,) = handle.stream_nemo_mel(1, spec, ld, [one])
    _same_bits(M.bits(single["mel"][:nm * mel_ld]), M.bits(together[0]["mel"][nm * mel_ld:2 * nm * mel_ld]), "alone against the middle of three")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def _refused(call, jobs, what):
    L = pkg("_lib")
    before = [{k: v.copy() for k, v in j.items() if isinstance(v, np.ndarray)} for j in jobs]
    with pytest.raises(L.CssError) as e:
        call(jobs)
    assert e.value.code == L.CSS_ERR_INVALID_ARG and "css_stream_nemo_" in str(e.value), (what, str(e.value))
    left = e.value.left[0] if isinstance(e.value.left, tuple) else e.value.left
    for j, b, l in zip(jobs, before, left):
        for k, v in b.items():
            _same_bits(j[k].view(np.uint8), v.view(np.uint8), what + ": the caller's " + k)
            if k in l:
                _same_bits(l[k].view(np.uint8), v.reshape(-1).view(np.uint8), what + ": " + k + " as the call left it")
    if isinstance(e.value.left, tuple):
        assert (M.bits(e.value.left[1]) == R.CANARY).all(), what + ": the operand"


def test_refusals(handle):
    c = next(c for c in M.cases() if c["name"] == "pad3_seams")
    rounds = M.rounds_of(c)
    state = M.state0(c)
    for rnd in rounds[:3]:
        job = M.job_of(c, rnd, state)
        state = M.next_state(job, [M.append_round(job, k) for k in range(3)])
    job1 = M.job_of(c, rounds[3], state)
    assert job1["D1"] - 256 >= job1["D0"] and int(job1["st"][0]["A"]) > 0
    # (the round reads the ring from frame D0 / 256 - pad - 1 on: more than 4 frames, which the short ring below cannot hold)
    assert job1["t_g1"] - min(job1["t_g0"], max(job1["D0"] // 256 - job1["pad"] - 1, 0)) > 4
    n_op = M.nemo_rows(job1["D1"] - job1["D0"]) * 3 * 160 + 1024

    def app(**kw):
        j = _call_job(job1)
        j.update(kw)
        return [j]
    call = lambda jobs, n=n_op: handle.stream_nemo_append(jobs, R.canary(n))
    call(app())
    st_bad = job1["st"].copy()
    st_bad[1]["J"] += 1
    st_whisper = job1["st"].copy()
    st_whisper[0]["A"], st_whisper[0]["J"] = 210, 1      # (a state of an open Whisper stream: one frame at 201 samples; none here)
    st_neg = job1["st"].copy()
    st_neg[0]["A"] = -1
    xl = job1["xlast_in"]
    bad = [dict(S=0), dict(S=5), dict(pad=-1), dict(pad=4097), dict(gate_ld=48), dict(t_g1=job1["t_g0"] - 1), dict(D1=job1["D0"] - 256),
           dict(D0=job1["D0"] + 1), dict(out_base=-1), dict(out_ld=job1["out_ld"] - 1), dict(carry_ld=job1["out_base"] - job1["D0"] - 1),
           dict(D1=job1["D1"] + 256), dict(gate_ld=4, gate=job1["gate"][:, :4].copy()), dict(st=st_bad), dict(st=st_whisper), dict(st=st_neg),
           dict(st=job1["st"][:2]), dict(gate=job1["gate"][:2]), dict(tail_in=job1["tail_in"][:, :-1]), dict(n_new=np.zeros(2, np.int32)),
           dict(act_out=R.canary8(3 * (job1["t_g1"] - job1["t_g0"]) - 1)), dict(drop=2), dict(closing=-1), dict(t_g0=-1), dict(D0=-256),
           dict(D1=job1["D0"] + (1 << 24) + 256), dict(preemphasis=1.0), dict(preemphasis=-0.5), dict(preemphasis=float("nan")),
           dict(preemphasis=float("inf")), dict(xlast_in=xl[:2]), dict(xlast_out=R.canary(2)), dict(tail_out=R.canary(3 * M.TAIL_LD - 1))]
    for kw in bad:
        _refused(call, app(**kw), f"append: {sorted(kw)}")
    _refused(lambda jobs: call(jobs, n_op - 1), app(), "append: operand one float short")
    _refused(lambda jobs: call(jobs, n_op + 1), app(), "append: operand one float long")
    _refused(lambda jobs: call(jobs, 2 * n_op - 1024), app() + app(S=2), "append: jobs with different S")
    _refused(lambda jobs: call(jobs, 65 * (n_op - 1024) + 1024), app() * 65, "append: 65 jobs")
    # ---- mel
    jobs, ld = _mel_jobs(1, 3)
    spec = np.zeros((514, ld), np.float32)
    mel = lambda **kw: [dict(jobs[0], mel=R.canary(jobs[0]["mel"].size), **kw)]
    mcall = lambda js, S=3, ld=ld: handle.stream_nemo_mel(S, spec, ld, js)
    mcall(mel())
    rows = jobs[0]["rows"]
    for kw in (dict(n_mels=64), dict(row0=-1), dict(rows=0), dict(row0=ld - 3 * rows + 1), dict(mel_ld=rows - 1),
               dict(n_new=np.array([1, -1, 2], np.int32)), dict(n_new=np.zeros(2, np.int32))):
        _refused(mcall, mel(**kw), f"mel: {sorted(kw)}")
    _refused(mcall, [dict(jobs[0], mel=R.canary(10))], "mel: a short mel")
    _refused(lambda js: mcall(js, S=0), mel(), "mel: S 0")
    _refused(lambda js: mcall(js, S=5), mel(), "mel: S 5")
    _refused(lambda js: mcall(js, ld=ld + 1), mel(), "mel: spec shorter than [514][ld]")
    _refused(mcall, mel() * 65, "mel: 65 jobs")
