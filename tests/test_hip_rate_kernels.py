"""Every launch form of csrc/resample.hip, through css_resample_host (include/css_mi355_rate.h) and the host entries of
include/css_mi355_rate_kernels.h, against the float64 reference and the elementwise bound of tests/rate_reference.py
(DESIGN.md 7b "The rate kernels' values").  Three kinds of assertion per launch:

  ownership  outputs and the slack behind them start as the canary 0x7FC0BEEF (int16: 0x5A5A); every element the launch does not
             own keeps its bits: behind n_m, behind the row ends up to dst_ld, before a column offset, the slack, the peak and
             clip words of rows that did not change
  value      |got - reference| <= P 2^-24 sum |x| |h| elementwise (0 where the span is silent: exactly +0.0f); the worst ratio of
             each test is printed; PCM16 with np.array_equal against rate_reference.pcm16
  bits       where two launches must agree: every table and session kernel against css_resample_host of the recording, a job in
             a table against the same job alone, the carried history against next_history

Coverage, one line per launch function:
  launch_resample                      test_resample_host: all thirteen ratios x float32, int16 x interleaved, planar x C 1, 2, 7, 8 at
                                       n_out 1, 2, P - 1, P, P + 1, 255 .. 257, 513, 1023 .. 1025, 2049 and an n_in below P;
                                       test_resample_host_large_lds: C 16 at 160/441 and 1/6, C 64 at 1/2, C 1 and 7 at 819/818 (above
                                       64 KiB at every C); test_resample_host_refuses_what_does_not_fit: 1/3 at C 64 and 48, C 47 runs
  launch_stream_ingest_resample_multi  test_stream_ingest: 1/3, 160/441, 320/441, 2/1, 1/6 x C 1, 7 x int16, float32 x interleaved,
                                       planar; pieces of 1, 7, 8, 9, 63, 257, the rest and the flush; source offsets 0, 1, 3, 7,
                                       destination columns 0 .. 3; test_stream_ingest_table: 17 mixed jobs, one of them 1/6 at C 16
                                       (above 64 KiB), each against the job alone
  launch_session_ingest_multi          test_session_ingest: the same ratios x C 1, 7, 8 and 1/6 at C 16 (above 64 KiB): a table of 9
                                       recordings, the level word at n_peak 0, 1, 256, n_m, preset below and above
  launch_stream_output_multi           test_stream_output: the five playback ratios, 1/2, 1/1 and 819/818 (above 64 KiB) x S 1, 3 x
                                       float32, PCM16; rounds of 1, 255, 256, 257, 4000 and the finishing round;
                                       test_stream_output_tile_edges: n_m 1023, 1024, 1025, 2049; test_stream_output_pcm16_planted;
                                       test_stream_output_table: 17 mixed jobs against each alone
  launch_session_output                test_session_output: the same ratios x S 1, 3 at n_m 1, P - 1, 1023, 1024, 1025, 2049, src_ld > n
  the entries' refusals                test_refusals
Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

import rate_reference as R
from conftest import pkg

pytestmark = pytest.mark.gpu

SLACK = 64                   # elements of slack behind every output
_id = lambda r: f"{r[0]}_{r[1]}"


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
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    if a.size == 0:
        return
    ua, ub = a.view(np.uint8).reshape(a.shape + (-1,)), b.view(np.uint8).reshape(b.shape + (-1,))
    diff = np.argwhere((ua != ub).any(axis=-1))
    assert diff.size == 0, (what, f"{len(diff)} values differ, the first at {tuple(diff[0])}")


def _all_canary(a, what):
    a = np.ascontiguousarray(a)
    stray = np.flatnonzero(a.reshape(-1) != R.CANARY16) if a.dtype == np.int16 else np.flatnonzero(R.bits(a).reshape(-1) != R.CANARY)
    assert stray.size == 0, (what, f"{stray.size} elements the launch does not own were written, the first at {stray[0]}")


def _ratio(got, ref, bound, what):
    """the worst |got - ref| / bound; a zero bound asks for +0.0f"""
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(R.bits(got)[bound == 0] == 0), (what, "a silent span did not come out as +0.0f")
    r = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    worst = np.unravel_index(int(r.argmax()), r.shape)
    assert r[worst] <= 1.0, (what, f"ratio {r[worst]:.3f} at {worst}: error {err[worst]!r}, bound {bound[worst]!r}")
    return float(r[worst])


class _Worst:
    """the worst ratio of a test and the case that produced it"""

    def __init__(self):
        self.r, self.what = 0.0, "-"

    def take(self, got, ref, bound, what):
        r = _ratio(got, ref, bound, what)
        if r > self.r:
            self.r, self.what = r, what
        return r

    def __str__(self):
        return f"{self.r:.3f} [{self.what}]"


def _fbits(v):
    return int(np.float32(v).view(np.uint32))


# ---- css_resample_host (resample_kernel) --------------------------------------------------------------------------------------------

def _host(handle, x, up, down, planar, what="css_resample_host", cap_rows=None):
    """css_resample_host of x [C, n] (interleaved: its transpose copied; planar: x itself with channel_stride n) -> [C, n_out]
    after the ownership check of the slack behind the n_out * C floats"""
    L = pkg("_lib")
    C_, n = x.shape
    m = R.count(up, down, n)
    src = np.ascontiguousarray(x if planar else x.T)
    out = R.canary(m * C_ + SLACK)
    n_out = C.c_int64(-1)
    ss, cs = (1, n) if planar else (C_, 1)
    rc = L.load().css_resample_host(handle.h, src.ctypes.data_as(C.c_void_p), int(x.dtype == np.int16), n, C_, ss, cs, up, down,
                                    out.ctypes.data_as(C.c_void_p), m + SLACK // C_ if cap_rows is None else cap_rows, C.byref(n_out))
    L.check(handle.h, rc)
    assert n_out.value == m, (what, n_out.value, m)
    _all_canary(out[m * C_:], what + ": behind n_out * C")
    return np.ascontiguousarray(out[:m * C_].reshape(m, C_).T)


@pytest.mark.parametrize("ratio", R.RATIOS, ids=_id)
def test_resample_host(handle, ratio):
    """The recordings of rate_reference.cases() (8 channels; C channels are the first C), both types, both layouts"""
    up, down = ratio
    worst, n_launch = _Worst(), 0
    for c in (c for c in R.cases() if (c.up, c.down) == ratio and c.H == 0 and c.C == 8):
        x8, _ = R.case_data(c)
        ref, bound = R.recording(x8, up, down)
        for C_ in (1, 2, 7, 8):
            x = np.ascontiguousarray(x8[:C_])
            got = _host(handle, x, up, down, False, c.name)
            worst.take(got, ref[:C_], bound[:C_], f"{c.name} C {C_} interleaved")
            _same_bits(_host(handle, x, up, down, True, c.name), got, f"{c.name} C {C_}: planar against interleaved")
            n_launch += 2
    assert n_launch >= 2 * 4 * 2 * 6       # (at 6/1 the fourteen counts are reached by seven lengths)
    print(f"resample_kernel {up}/{down}: {n_launch} launches, worst error / bound {worst}")


@pytest.mark.parametrize("ratio,C_", R.LARGE_LDS, ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_resample_host_large_lds(handle, ratio, C_):
    """Launches whose dynamic LDS is above 64 KiB, n_out at the tile's edges and two tiles + 1"""
    up, down = ratio
    lds = R.lds_bytes(up, down, C_)
    assert 65536 < lds <= 160 * 1024
    assert (R.lds_bytes(160, 441, 16), R.lds_bytes(1, 6, 16), R.lds_bytes(1, 2, 64), R.lds_bytes(1, 3, 64)) == (86784, 109860, 146340, 219124)
    worst, n_launch = _Worst(), 0
    for c in (c for c in R.cases() if (c.up, c.down) == ratio and c.C == C_ and c.name.startswith("large")):
        x, _ = R.case_data(c)
        ref, bound = R.recording(x, up, down)
        got = _host(handle, x, up, down, False, c.name)
        worst.take(got, ref, bound, c.name)
        _same_bits(_host(handle, x, up, down, True, c.name), got, c.name + ": planar against interleaved")
        n_launch += 2
    assert n_launch == 8 and worst.r > 0.0
    print(f"resample_kernel {up}/{down} C {C_} ({lds} B of LDS): worst error / bound {worst}")


def test_resample_host_refuses_what_does_not_fit(handle):
    """1/3 with 64 channels needs 219,124 B: CSS_ERR_INVALID_ARG, out and n_out untouched"""
    L = pkg("_lib")
    x = R.samples(64, 100, np.float32, 1)
    with pytest.raises(L.CssError) as e:
        _host(handle, x, 1, 3, True)
    assert e.value.code == L.CSS_ERR_INVALID_ARG and "rate ratio" in e.value.text
    out, n_out = R.canary(64 * 40), C.c_int64(-5)
    src = np.ascontiguousarray(x.T)
    rc = L.load().css_resample_host(handle.h, src.ctypes.data_as(C.c_void_p), 0, 100, 64, 64, 1, 1, 3, out.ctypes.data_as(C.c_void_p), 40,
                                    C.byref(n_out))
    assert rc == L.CSS_ERR_INVALID_ARG and n_out.value == -5
    _all_canary(out, "a refused call")
    # the rule's edge at 1/3: 47 channels fit the 160 KiB (160,984 B), 48 do not
    assert R.lds_bytes(1, 3, 47) <= 160 * 1024 < R.lds_bytes(1, 3, 48)
    ref, bound = R.recording(x[:47], 1, 3)
    worst = _ratio(_host(handle, x[:47], 1, 3, True), ref, bound, "1/3 C 47")
    print(f"resample_kernel 1/3 C 47 ({R.lds_bytes(1, 3, 47)} B of LDS): worst error / bound {worst:.3f}")
    with pytest.raises(L.CssError):
        _host(handle, x[:48], 1, 3, True)


# ---- stream ingest --------------------------------------------------------------------------------------------------------------------

def _layout(x, planar, pad=0):
    """x [C, n] as the job's src: (array, plane_ld)"""
    if planar:
        a = np.zeros((x.shape[0], x.shape[1] + pad), x.dtype)
        a[:, :x.shape[1]] = x
        return a.reshape(-1), x.shape[1] + pad
    return np.ascontiguousarray(x.T).reshape(-1), 0


def _ingest_job(x, hist, N0, m0, n_m, up, down, planar, src_offset, dst_col, flush):
    """(job dict, dst_ld) of one stream-ingest job on piece x [C, n]"""
    C_, n = x.shape
    src, plane_ld = _layout(x, planar, pad=3)
    dst_ld = dst_col + n_m + 5
    return dict(src=src if n else np.zeros(0, x.dtype), hist_in=hist, hist_out=None if flush else R.canary(hist.shape),
                dst=R.canary(dst_col + C_ * dst_ld + SLACK), up=up, down=down, C=C_, src_offset=src_offset, H=hist.shape[1], dst_col=dst_col,
                plane_ld=plane_ld if n else 0, n=n, N0=N0, m0=m0, n_m=n_m, dst_ld=dst_ld), dst_ld


def _ingest_owned(dst, C_, dst_col, dst_ld, n_m, what):
    """the owned block [C, n_m] of a stream-ingest dst after the ownership checks"""
    _all_canary(dst[:dst_col], what + ": before the column offset")
    rows = dst[dst_col:dst_col + C_ * dst_ld].reshape(C_, dst_ld)
    _all_canary(rows[:, n_m:], what + ": behind n_m up to dst_ld")
    _all_canary(dst[dst_col + C_ * dst_ld:], what + ": the slack")
    return rows[:, :n_m]


def _stream_ingest(handle, whole, up, down, planar, turn, what, worst):
    """the recording through the jobs of rate_reference.stream_jobs, one launch each, history carried; returns [C, count]"""
    C_ = whole.shape[0]
    hist = np.zeros((C_, R.history_len(up, down)), np.float32)
    outs = []
    for k, (N0, n, m0, n_m, H, flush) in enumerate(R.stream_jobs(up, down, whole.shape[1])):
        piece = whole[:, N0:N0 + n]
        src_offset, dst_col = (0, 1, 3, 7)[(k + turn) % 4], (k + turn // 4) % 4
        w = f"{what} job {k} (N0 {N0} n {n} m0 {m0} n_m {n_m} src_offset {src_offset} dst_col {dst_col})"
        job, dst_ld = _ingest_job(piece, hist, N0, m0, n_m, up, down, planar, src_offset, dst_col, flush)
        (dst, hist_out, _), = handle.rate_ingest(0, [job])
        got = _ingest_owned(dst, C_, dst_col, dst_ld, n_m, w)
        ref, bound = R.reference(piece, hist, N0, m0, n_m, up, down)
        worst.take(np.ascontiguousarray(got), ref, bound, w)
        outs.append(got)
        if flush:
            assert hist_out is None
        else:
            nxt = R.next_history(hist, piece)
            _same_bits(hist_out.reshape(C_, H), nxt, w + ": the carried history")
            hist = nxt
    return np.concatenate(outs, axis=1)


@pytest.mark.parametrize("ratio", R.STREAM_INGEST_RATIOS, ids=_id)
def test_stream_ingest(handle, ratio):
    """Pieces of 1, 7, 8, 9, 63 and 257 inputs (all shorter than H at 1/3 and 1/6; the first have n_m = 0 and N0 - H < 0 and
    still write their history), the rest, and the flush (no hist_out; the inputs past the piece are zeros)"""
    up, down = ratio
    worst, turn = _Worst(), 0
    n_in = R.job_recording_len(up, down)
    assert R.stream_jobs(up, down, n_in)[0][3] == 0
    for C_ in (1, 7):
        for dtype in (np.float32, np.int16):
            whole = R.samples(C_, n_in, dtype, 40 + C_)
            host = _host(handle, whole, up, down, True)
            for planar in (False, True):
                what = f"{up}/{down} C {C_} {np.dtype(dtype).name} {'planar' if planar else 'interleaved'}"
                got = _stream_ingest(handle, whole, up, down, planar, turn, what, worst)
                _same_bits(got, host, what + ": the pieces against css_resample_host of the recording")
                turn += 1
    print(f"stream_ingest_resample_kernel {up}/{down}: worst error / bound {worst}")


def _mixed_ingest_jobs():
    """17 jobs of mixed ratio, C, type and layout, cut from recordings mid-stream; one is 1/6 with 16 channels"""
    jobs = []
    for k in range(17):
        up, down = R.STREAM_INGEST_RATIOS[k % 5]
        C_ = 16 if k == 9 else (1, 7, 2, 8)[k % 4]
        assert k != 9 or (up, down) == (1, 6)
        dtype = np.int16 if k % 2 else np.float32
        whole = R.samples(C_, R.job_recording_len(up, down), dtype, 300 + k)
        N0, n, m0, n_m, H, flush = R.stream_jobs(up, down, whole.shape[1])[3 + k % 5]
        hist = R.history_of(whole, N0, H)
        job, dst_ld = _ingest_job(whole[:, N0:N0 + n], hist, N0, m0, n_m, up, down, k % 3 == 0, (0, 1, 3, 7)[k % 4], k % 4, flush)
        jobs.append((job, dst_ld, C_, k % 4, n_m))
    return jobs


def test_stream_ingest_table(handle):
    """One call with 17 entries (two launches, the first with the LDS of its largest entry, above 64 KiB) against 17 calls"""
    jobs = _mixed_ingest_jobs()
    together = handle.rate_ingest(0, [j[0] for j in jobs])
    n_hist = 0
    for k, ((job, dst_ld, C_, dst_col, n_m), (dst, hist_out, _)) in enumerate(zip(jobs, together)):
        (dst1, hist1, _), = handle.rate_ingest(0, [job])
        _same_bits(dst, dst1, f"job {k}: dst in the table against alone")
        _ingest_owned(dst, C_, dst_col, dst_ld, n_m, f"job {k} in the table")
        assert (hist_out is None) == (hist1 is None)
        if hist_out is not None:
            _same_bits(hist_out, hist1, f"job {k}: hist_out in the table against alone")
            n_hist += 1
    assert n_hist >= 10 and sum(j[4] > 0 for j in jobs) >= 10


# ---- session ingest -------------------------------------------------------------------------------------------------------------------

SESSION_INGEST = [(r, C_) for r in R.STREAM_INGEST_RATIOS for C_ in (1, 7, 8)] + [((1, 6), 16)]


@pytest.mark.parametrize("ratio,C_", SESSION_INGEST, ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_session_ingest(handle, ratio, C_):
    """A table of 9 recordings (two launches) of different lengths, one a single input sample; dst [n_m][C] and the level word"""
    up, down = ratio
    _, _, P = R.geometry(up, down)
    n_ins = [1] + [R.n_in_for(up, down, m) for m in (2, P - 1, R.RS_TILE - 1, R.RS_TILE, R.RS_TILE + 1, 2 * R.RS_TILE + 1, P + 1)] + [max(2, P // 2)]
    jobs, meta = [], []
    for k, n in enumerate(n_ins):
        x = R.samples(C_, n, np.int16 if k % 2 else np.float32, 700 + k)
        n_m = R.count(up, down, n)
        src, plane_ld = _layout(x, k % 3 == 1, pad=1)
        n_peak = (0, 1, R.RS_TILE, n_m)[k % 4] if k < 8 else n_m + 10
        before = (0, _fbits(0.001), _fbits(7.5))[k % 3]       # nothing, below any maximum of more than a few samples, above every maximum
        jobs.append(dict(src=src, dst=R.canary(n_m * C_ + SLACK), up=up, down=down, C=C_, src_offset=(0, 1, 3, 7)[k % 4], plane_ld=plane_ld,
                         n=n, n_m=n_m, n_peak=n_peak, level_before=before))
        meta.append((x, n_m, n_peak, before))
    worst = _Worst()
    for k, ((x, n_m, n_peak, before), (dst, _, level)) in enumerate(zip(meta, handle.rate_ingest(1, jobs))):
        what = f"{up}/{down} C {C_} recording {k} (n_in {x.shape[1]}, n_m {n_m}, n_peak {n_peak})"
        _all_canary(dst[n_m * C_:], what + ": behind n_m * C")
        got = np.ascontiguousarray(dst[:n_m * C_].reshape(n_m, C_).T)
        ref, bound = R.recording(x, up, down)
        worst.take(got, ref, bound, what)
        _same_bits(got, _host(handle, x, up, down, False), what + ": against css_resample_host")
        scanned = got[:, :min(n_peak, n_m)]
        peak = _fbits(np.max(np.abs(scanned))) if scanned.size else 0
        assert level == max(before, peak), (what, hex(level), hex(before), hex(peak))       # (float bits of values >= 0 order as the values)
    print(f"session_ingest_resample_kernel {up}/{down} C {C_}: worst error / bound {worst}")


# ---- stream output --------------------------------------------------------------------------------------------------------------------

OUT_RATIOS = R.OUT_RATIOS + ((1, 2), (1, 1), R.EDGE_RATIO)
ROUNDS = (1, 255, 256, 257, 4000)


def _out_count(up, down, n, finished):
    return n if up == down else R.count(up, down, n, finished)


def _output_job(rows, hist, N0, m0, n_m, up, down, pcm16, gain, flush, peak, clipped, src_ld=None):
    S, n = rows.shape
    src_ld = n + 3 if src_ld is None else src_ld
    src = np.full((S, src_ld), np.float32(np.nan))       # what lies in a row behind n must not be read
    src[:, :n] = rows
    per = 8 if pcm16 else 4
    dst_ld = (n_m + 5 + per - 1) // per * per
    dst = R.canary16(S * dst_ld + SLACK) if pcm16 else R.canary(S * dst_ld + SLACK)
    return dict(src=src, hist_in=hist, hist_out=None if flush or not hist.size else R.canary(hist.shape), dst=dst, up=up, down=down,
                H=hist.shape[1], pcm16=int(pcm16), gain=gain, src_ld=src_ld, n=n, N0=N0, m0=m0, n_m=n_m, dst_ld=dst_ld, peak=peak,
                clipped=clipped), dst_ld


def _output_owned(dst, S, dst_ld, n_m, what):
    rows = dst[:S * dst_ld].reshape(S, dst_ld)
    _all_canary(rows[:, n_m:], what + ": behind n_m up to dst_ld")
    _all_canary(dst[S * dst_ld:], what + ": the slack")
    return np.ascontiguousarray(rows[:, :n_m])


def _expected_words(rows, peak, clipped, clips):
    """the peak words (raised only when larger; silence leaves them) and the clip counts after a round"""
    pk = [max(int(p), _fbits(np.max(np.abs(r))) if r.size else 0) for p, r in zip(peak, rows)]
    return np.array(pk, np.uint32), np.asarray(clipped, np.uint64) + np.asarray(clips, np.uint64)


@pytest.mark.parametrize("S", (1, 3))
@pytest.mark.parametrize("ratio", OUT_RATIOS, ids=_id)
def test_stream_output(handle, ratio, S):
    """Rounds of 1, 255, 256, 257 and 4000 final samples with carried history, then the finishing round (no hist_out) that completes
    the count to ceil(n up / down); float32 and PCM16 (gain 0.9 on samples up to 1.2, so the clamp works); a round of silence at
    the end of the PCM16 pass must leave the peak words alone"""
    up, down = ratio
    unity = up == down
    whole = (R.samples(S, sum(ROUNDS), np.float32, 900 + S) * np.float32(1.2)).astype(np.float32)
    host = whole.copy() if unity else _host(handle, whole, up, down, True)
    ref, bound = (whole.astype(np.float64), np.zeros(whole.shape)) if unity else R.recording(whole, up, down)
    H = 0 if unity else R.history_len(up, down)
    worst = _Worst()
    for pcm16, gain in ((0, 1.0), (1, 0.9)):
        hist = np.zeros((S, H), np.float32)
        peak = np.array([0, _fbits(0.05), _fbits(9.0)][:S], np.uint32)
        clipped = np.array([0, 5, 1 << 40][:S], np.uint64)
        N0, m0 = 0, 0
        for k, (n, flush) in enumerate([(k, False) for k in ROUNDS] + ([] if unity else [(0, True)])):
            rows = whole[:, N0:N0 + n]
            m1 = _out_count(up, down, N0 + n, flush)
            n_m = m1 - m0
            what = f"{up}/{down} S {S} pcm16 {pcm16} round {k} (N0 {N0} n {n} m0 {m0} n_m {n_m})"
            job, dst_ld = _output_job(rows, hist, N0, m0, n_m, up, down, pcm16, gain, flush, peak, clipped)
            (dst, hist_out, peak_after, clipped_after), = handle.rate_output(0, S, [job])
            got = _output_owned(dst, S, dst_ld, n_m, what)
            want = host[:, m0:m0 + n_m]
            clips = [0] * S
            if pcm16:
                q, _ = R.pcm16(want, gain)
                clips = [R.pcm16(r, gain)[1] for r in want]
                assert np.array_equal(got, q), what
            else:
                _same_bits(got, want, what + ": against css_resample_host of the rows")
                if not unity:
                    piece_ref, piece_bound = R.reference(rows, hist, N0, m0, n_m, up, down)
                    assert np.array_equal(piece_ref, ref[:, m0:m0 + n_m])
                    worst.take(got, piece_ref, piece_bound, what)
            pk, cl = _expected_words(rows, peak, clipped, clips)
            assert np.array_equal(peak_after, pk) and np.array_equal(clipped_after, cl), (what, peak_after, pk, clipped_after, cl)
            peak, clipped = pk, cl
            if hist_out is not None:
                nxt = R.next_history(hist, rows)
                _same_bits(hist_out.reshape(S, H), nxt, what + ": the carried history")
                hist = nxt
            else:
                assert flush or unity
            N0, m0 = N0 + n, m1
        assert m0 == host.shape[1] and (not pcm16 or int(clipped[0]) > 0)
        # a recording of silence: +0.0f (PCM16: 0) everywhere, and no word moves
        n_m = _out_count(up, down, 64, True)
        job, dst_ld = _output_job(np.zeros((S, 64), np.float32), np.zeros((S, H), np.float32), 0, 0, n_m, up, down, pcm16, gain, True, peak, clipped)
        (dst, _, peak_after, clipped_after), = handle.rate_output(0, S, [job])
        got = _output_owned(dst, S, dst_ld, n_m, "silence")
        assert not got.view(np.uint16 if pcm16 else np.uint32).any(), f"{up}/{down} pcm16 {pcm16}: silence is not +0"
        assert np.array_equal(peak_after, peak) and np.array_equal(clipped_after, clipped), f"{up}/{down} pcm16 {pcm16}: silence moved a word"
    print(f"stream_output_kernel {up}/{down} S {S}: worst error / bound {worst}")


@pytest.mark.parametrize("ratio", OUT_RATIOS, ids=_id)
def test_stream_output_tile_edges(handle, ratio):
    """n_m at SO_TILE - 1, SO_TILE, SO_TILE + 1 and two tiles + 1: whole recordings as one job (H 0, N0 0, m0 0)"""
    up, down = ratio
    worst = _Worst()
    for n_m in (R.SO_TILE - 1, R.SO_TILE, R.SO_TILE + 1, 2 * R.SO_TILE + 1):
        n = n_m if up == down else R.n_in_for(up, down, n_m)
        rows = R.samples(2, n, np.float32, n_m)
        job, dst_ld = _output_job(rows, np.zeros((2, 0), np.float32), 0, 0, n_m, up, down, 0, 1.0, True, np.zeros(2, np.uint32), np.zeros(2, np.uint64))
        (dst, _, peak, clipped), = handle.rate_output(0, 2, [job])
        what = f"{up}/{down} n_m {n_m}"
        got = _output_owned(dst, 2, dst_ld, n_m, what)
        if up == down:
            _same_bits(got, rows, what)
        else:
            ref, bound = R.recording(rows, up, down)
            worst.take(got, ref[:, :n_m], bound[:, :n_m], what)
            _same_bits(got, _host(handle, rows, up, down, True)[:, :n_m], what + ": against css_resample_host")
        assert list(peak) == [_fbits(np.max(np.abs(r))) for r in rows] and not clipped.any()
    print(f"stream_output_kernel {up}/{down} at the tile's edges: worst error / bound {worst}")


@pytest.mark.parametrize("what,gain", R.PCM_CASES)
def test_stream_output_pcm16_planted(handle, what, gain):
    """1/1: the encoder alone on rate_reference.pcm_samples -- the ties +-0.5 -> +-16384, +-1.0, both float32 neighbours of
    32767.5 / 32767, values beyond +-1.0001 -- bit for bit and with the clip counts, on top of counts from before"""
    y = R.pcm_samples(gain)
    rows = np.stack([y, -y, y[::-1]])
    before = np.array([0, 3, 1 << 33], np.uint64)
    job, dst_ld = _output_job(rows, np.zeros((3, 0), np.float32), 0, 0, y.size, 1, 1, 1, gain, True, np.zeros(3, np.uint32), before)
    (dst, _, peak, clipped), = handle.rate_output(0, 3, [job])
    got = _output_owned(dst, 3, dst_ld, y.size, what)
    for k in range(3):
        q, clips = R.pcm16(rows[k], gain)
        assert np.array_equal(got[k], q), (what, k, np.flatnonzero(got[k] != q)[:5])
        assert int(clipped[k]) == int(before[k]) + clips and clips > 0, (what, k)
    if gain == 1.0:
        assert list(got[0, :4]) == [16384, -16384, 32767, -32767]
    assert list(peak) == [_fbits(np.max(np.abs(y)))] * 3


def test_stream_output_table(handle):
    """One call with 17 entries (two launches; the first holds 819/818, above 64 KiB) against 17 calls, S = 2"""
    jobs = []
    for k in range(17):
        up, down = OUT_RATIOS[k % len(OUT_RATIOS)]
        n, N0 = (300, 1500, 40, 1030)[k % 4], 2000 + 13 * k
        whole = R.samples(2, N0 + n, np.float32, 1200 + k) * np.float32(1.1)
        H = 0 if up == down else R.history_len(up, down)
        m0 = _out_count(up, down, N0, False)
        n_m = _out_count(up, down, N0 + n, False) - m0
        hist = R.history_of(whole, N0, H)
        jobs.append(_output_job(whole[:, N0:], hist, N0, m0, n_m, up, down, k % 2, 0.8 + 0.05 * k, k % 5 == 4, np.array([k, _fbits(0.5)], np.uint32),
                                np.array([k, 0], np.uint64)) + (n_m,))
    together = handle.rate_output(0, 2, [j[0] for j in jobs])
    for k, ((job, dst_ld, n_m), left) in enumerate(zip(jobs, together)):
        alone, = handle.rate_output(0, 2, [job])
        _output_owned(left[0], 2, dst_ld, n_m, f"job {k} in the table")
        for a, b, name in zip(left, alone, ("dst", "hist_out", "peak", "clipped")):
            assert (a is None) == (b is None)
            if a is not None:
                _same_bits(a, b, f"job {k}: {name} in the table against alone")
    assert sum(j[2] > 0 for j in jobs) == 17


# ---- session output -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", (1, 3))
@pytest.mark.parametrize("ratio", R.OUT_RATIOS + ((1, 2), R.EDGE_RATIO), ids=_id)
def test_session_output(handle, ratio, S):
    """Rows of n samples in an allocation of src_ld = n + 9 with NaNs behind n (the kernel reads zeros there); peak words of the
    OUTPUT samples, on top of words below and above them"""
    up, down = ratio
    _, _, P = R.geometry(up, down)
    worst = _Worst()
    for n_m in (1, P - 1, R.SO_TILE - 1, R.SO_TILE, R.SO_TILE + 1, 2 * R.SO_TILE + 1):
        n = R.n_in_for(up, down, n_m)
        n_m = R.count(up, down, n)       # (a ratio above 1 reaches some counts only from above)
        rows = R.samples(S, n, np.float32, 1500 + n_m)
        before = np.array([0, _fbits(0.01), _fbits(50.0)][:S], np.uint32)
        job, dst_ld = _output_job(rows, np.zeros((S, 0), np.float32), 0, 0, n_m, up, down, 0, 1.0, True, before, np.zeros(S, np.uint64), src_ld=n + 9)
        job.pop("hist_out")
        (dst, _, peak, _), = handle.rate_output(1, S, [job])
        what = f"{up}/{down} S {S} n {n} n_m {n_m}"
        got = _output_owned(dst, S, dst_ld, n_m, what)
        ref, bound = R.recording(rows, up, down)
        worst.take(got, ref, bound, what)
        _same_bits(got, _host(handle, rows, up, down, True), what + ": against css_resample_host")
        assert list(peak) == [max(int(b), _fbits(np.max(np.abs(g)))) for b, g in zip(before, got)], what
    print(f"session_output_kernel {up}/{down} S {S}: worst error / bound {worst}")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def _refused(call, jobs, what, arrays):
    """the call raises CSS_ERR_INVALID_ARG with a message, and every array it was handed keeps its bits"""
    L = pkg("_lib")
    with pytest.raises(L.CssError) as e:
        call(jobs)
    assert e.value.code == L.CSS_ERR_INVALID_ARG and e.value.text, what
    for job, left in zip(jobs, e.value.left):
        for name, a in zip(arrays, left):
            if isinstance(a, np.ndarray) and job.get(name) is not None:
                _same_bits(a, np.ascontiguousarray(job[name]).reshape(-1), f"{what}: {name} after the refusal")
    return e.value.text


def test_refusals(handle):
    """Each entry refuses each item of the header's list before anything is launched or written"""
    x = R.samples(2, 100, np.float32, 3)
    H = R.history_len(1, 3)
    hist = R.history_of(x, 50, H)

    def ingest(form, **change):
        n_m = 10
        job, _ = _ingest_job(x[:, 50:], hist, 50, 0, n_m, 1, 3, False, 0, 0, form == 1)
        if form == 1:
            job.update(dst_ld=0, dst=R.canary(2 * n_m + SLACK))
        arrays = {k: change.pop(k) for k in list(change) if k in ("src", "hist_in", "hist_out", "dst")}
        job.update(change)
        job.update(arrays)
        return [job]

    for form in (0, 1):
        call = lambda jobs, form=form: handle.rate_ingest(form, jobs)
        names = ("dst", "hist_out")
        handle.rate_ingest(form, ingest(form))       # (the unchanged job is accepted)
        for what, change in (("up == down", dict(up=1, down=1)), ("not in lowest terms", dict(up=2, down=6)), ("P above 128", dict(up=1, down=7)),
                             ("L above 16384", dict(up=820, down=1)), ("up 0", dict(up=0)), ("C 0", dict(C=0)), ("C 65", dict(C=65)),
                             ("negative H", dict(H=-1)), ("negative n", dict(n=-1)), ("negative n_m", dict(n_m=-1)),
                             ("m0 + n_m overflows", dict(m0=(1 << 62))), ("m0 above 2^40", dict(m0=(1 << 40) + 1)),
                             ("src_offset 8", dict(src_offset=8)), ("src short", dict(src=x[:, 50:].T.reshape(-1)[:-1].copy())),
                             ("hist short", dict(hist_in=hist.reshape(-1)[:-1].copy(), hist_out=None)),
                             ("dst short", dict(dst=R.canary(2 * 10 - 1 if form else 15 + 9))), ("plane_ld below n", dict(plane_ld=49))):
            _refused(call, ingest(form, **change), f"ingest form {form}: {what}", names)
        wide = R.samples(64, 100, np.float32, 4)
        job, _ = _ingest_job(wide, np.zeros((64, 0), np.float32), 0, 0, 5, 1, 3, False, 0, 0, True)
        if form == 1:
            job.update(dst_ld=0)
        assert "LDS" in _refused(call, [job], f"ingest form {form}: 1/3 at C 64 does not fit", names)
    _refused(lambda jobs: handle.rate_ingest(0, jobs), ingest(0, dst_col=4), "ingest form 0: dst_col 4", ("dst", "hist_out"))
    _refused(lambda jobs: handle.rate_ingest(0, jobs), ingest(0, dst_ld=9), "ingest form 0: dst_ld below n_m", ("dst", "hist_out"))
    _refused(lambda jobs: handle.rate_ingest(1, jobs), ingest(1, dst_ld=16), "ingest form 1: dst_ld set", ("dst", "hist_out"))
    _refused(lambda jobs: handle.rate_ingest(2, jobs), ingest(0), "ingest: form 2", ("dst", "hist_out"))
    _refused(lambda jobs: handle.rate_ingest(0, jobs), ingest(0) * 65, "ingest: 65 jobs", ("dst", "hist_out"))

    rows = R.samples(2, 100, np.float32, 5)
    Ho = R.history_len(3, 1)

    def output(form, **change):
        h = np.zeros((2, 0), np.float32) if form else R.history_of(rows, 40, Ho)
        job, _ = _output_job(rows[:, 40:] if not form else rows, h, 0 if form else 40, 0, 24, 3, 1, 0, 1.0, bool(form), np.zeros(2, np.uint32),
                             np.zeros(2, np.uint64))
        arrays = {k: change.pop(k) for k in list(change) if k in ("src", "hist_in", "hist_out", "dst", "peak", "clipped")}
        job.update(change)
        job.update(arrays)
        return [job]

    names = ("dst", "hist_out", "peak", "clipped")
    for form in (0, 1):
        call = lambda jobs, form=form: handle.rate_output(form, 2, jobs)
        handle.rate_output(form, 2, output(form))
        for what, change in (("up == down == 2", dict(up=2, down=2)), ("not in lowest terms", dict(up=6, down=2)), ("L above 16384", dict(up=820, down=1)),
                             ("down 0", dict(down=0)), ("negative n", dict(n=-1)), ("negative n_m", dict(n_m=-1)), ("n_m above 2^24", dict(n_m=(1 << 24) + 1)),
                             ("dst_ld not a multiple of 16 bytes", dict(dst_ld=30)), ("dst_ld below n_m", dict(dst_ld=20)),
                             ("src_ld below n", dict(src_ld=50)), ("src short", dict(src=np.zeros(100, np.float32))),
                             ("dst short", dict(dst=R.canary(32 + 23)))):
            _refused(call, output(form, **change), f"output form {form}: {what}", names)
    call0 = lambda jobs: handle.rate_output(0, 2, jobs)
    _refused(call0, output(0, H=-1), "output form 0: negative H", names)
    _refused(call0, output(0, hist_in=np.zeros(2 * Ho - 1, np.float32), hist_out=None), "output form 0: hist short", names)
    _refused(call0, output(0, m0=1 << 62), "output form 0: m0 + n_m overflows", names)
    _refused(call0, output(0, up=1, down=1, n_m=61), "output form 0: 1/1 with n_m above n", names)
    _refused(call0, output(0, pcm16=1, dst=R.canary16(2 * 36 + SLACK), dst_ld=36), "output form 0: PCM16 rows of 72 bytes", names)
    _refused(lambda jobs: handle.rate_output(1, 2, jobs), output(1, m0=1), "output form 1: m0 set", names)
    _refused(lambda jobs: handle.rate_output(1, 2, jobs), output(1) * 2, "output form 1: two jobs", names)
    _refused(lambda jobs: handle.rate_output(0, 65, jobs), output(0, peak=np.zeros(65, np.uint32), clipped=np.zeros(65, np.uint64)), "output: S 65", names)
    _refused(lambda jobs: handle.rate_output(0, 0, jobs), output(0, peak=np.zeros(0, np.uint32), clipped=np.zeros(0, np.uint64)), "output: S 0", names)


def test_refusal_of_a_shared_history_array(handle):
    """hist_out must be another array than hist_in: the binding copies hist_out, so the two are given the same address by hand"""
    L = pkg("_lib")
    x = np.ascontiguousarray(R.samples(1, 80, np.float32, 6).reshape(-1))
    H = R.history_len(1, 3)
    hist = np.full(H, 0.25, np.float32)
    dst = R.canary(64)
    j = (L.CssRateIngestJob * 1)()
    j[0].up, j[0].down, j[0].C, j[0].H, j[0].has_hist_out = 1, 3, 1, H, 1
    j[0].n, j[0].N0, j[0].n_m, j[0].dst_ld = 80, 100, 8, 8
    j[0].src_elems, j[0].hist_elems, j[0].dst_floats = 80, H, 64
    j[0].src, j[0].hist_in, j[0].hist_out, j[0].dst = x.ctypes.data, hist.ctypes.data, hist.ctypes.data, dst.ctypes.data
    assert L.load().css_rate_ingest_host(handle.h, 0, j, 1) == L.CSS_ERR_INVALID_ARG
    assert b"another array" in L.load().css_last_error(handle.h)
    _all_canary(dst, "a refused call")
    assert (hist == 0.25).all()
    o = (L.CssRateOutputJob * 1)()
    peak, clipped = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    o[0].up, o[0].down, o[0].H, o[0].has_hist_out, o[0].gain = 3, 1, H, 1, 1.0
    o[0].src_ld, o[0].n, o[0].N0, o[0].n_m, o[0].dst_ld = 80, 80, 100, 8, 8
    o[0].src_floats, o[0].hist_elems, o[0].dst_elems = 80, H, 64
    o[0].src, o[0].hist_in, o[0].hist_out, o[0].dst = x.ctypes.data, hist.ctypes.data, hist.ctypes.data, dst.ctypes.data
    o[0].peak, o[0].clipped = peak.ctypes.data, clipped.ctypes.data
    assert L.load().css_rate_output_host(handle.h, 0, 1, o, 1) == L.CSS_ERR_INVALID_ARG
    assert b"another array" in L.load().css_last_error(handle.h)
    _all_canary(dst, "a refused call")
