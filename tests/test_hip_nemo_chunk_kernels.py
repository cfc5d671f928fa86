"""The two kernels behind NeMo chunks on caller data, on the MI355X (include/css_mi355_nemo_chunk.h: css_nemo_chunk_host,
css_stream_nemo_mel_history_host; csrc/nemo_stream.hip nemo_chunk_kernel and the ring write of nemo_mel_multi_kernel), against the
exact model of tests/nemo_chunk_reference.py: outputs, mean and std bit for bit, canaries wherever nothing may be written."""
import numpy as np
import pytest

import nemo_chunk_reference as M
from conftest import pkg

pytestmark = pytest.mark.gpu

SLACK = 64
CANARY16 = 0xBEEF
RAW, PER_FEATURE, F32, F16 = 0, 1, 0, 1


@pytest.fixture(scope="module")
def handle():
    L = pkg("_lib")
    if L.load().css_device_count() < 1:
        pytest.fail("no HIP device visible")
    w = pkg("weights")
    sep = pkg("separator").HipSeparator(w.apply_golden_recipe(w.portable_state_dict(w.ModelDesc(num_blocks=1), 5)), None, device=0)
    yield sep.handle
    sep.close()


def _words(a):
    """an array as unsigned words of its element size"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.itemsize == 2 else np.uint32)


def _job(values, hist, first, end, width, normalize, dtype, pad=0.0, ld=None, off=0):
    """a chunk job over `values` [n_mels][n] as frames [first, first + n) of a ring of `hist` slots that ends at frame `end`: every
    other slot of the ring holds a canary (a NaN: a kernel that read one would show it), out and the statistics are canaries"""
    n_mels, n = values.shape
    assert first >= max(end - hist, 0) and first + n <= end
    ring = np.tile(M.canary(hist), (n_mels, 1))
    ring[:, (first + np.arange(n)) % hist] = values
    ld = width if ld is None else ld
    size = off + n_mels * ld + SLACK
    out = np.full(size, CANARY16, np.uint16) if dtype == F16 else M.canary(size)
    return dict(n_mels=n_mels, n_frames=n, width=width, dtype=dtype, normalize=normalize, pad_value=pad, hist=hist, end_frame=end,
                first_frame=first, ld=ld, out_offset=off, ring=ring, out=out, mean=M.canary(n_mels), std=M.canary(n_mels))


def _check(job, got, values, what):
    """one job's results against the model: the chunk, the statistics, canaries everywhere else"""
    n_mels, ld, off, width = job["n_mels"], job["ld"], job["out_offset"], job["width"]
    want, mean, std = M.chunk(values, width, job["normalize"] == PER_FEATURE, np.float16 if job["dtype"] == F16 else np.float32, job["pad_value"])
    out = _words(got["out"])
    blank = CANARY16 if job["dtype"] == F16 else M.CANARY
    rows = out[off:off + n_mels * ld].reshape(n_mels, ld)
    bad = np.argwhere(rows[:, :width] != _words(want))
    assert bad.size == 0, (what, "first differing (band, column)", bad[0].tolist(), len(bad))
    assert (rows[:, width:] == blank).all(), (what, "the rows' gaps")
    assert (out[:off] == blank).all() and (out[off + n_mels * ld:] == blank).all(), (what, "before and behind the rows")
    if job["normalize"] == PER_FEATURE:
        assert np.array_equal(M.bits(got["mean"]), M.bits(mean)) and np.array_equal(M.bits(got["std"]), M.bits(std)), (what, "mean / std")
    else:
        assert (M.bits(got["mean"]) == M.CANARY).all() and (M.bits(got["std"]) == M.CANARY).all(), (what, "a raw chunk's statistics")


# ---- the chunk kernel ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i,n", list(enumerate(M.N_FRAMES)), ids=lambda v: str(v))
def test_chunks_of_every_length(handle, i, n):
    """one table call per span length: both band counts, rings of 32, 33 and 3000 slots, spans that wrap and spans that do not,
    width n, n + 1 and 3000, ld > width, float16 at an odd element offset and float32 at a 4-byte-only offset, both modes"""
    jobs, vals = [], []
    for n_mels in (80, 128):
        values = M.frames(n_mels, n, 20 + i, "mixed" if n >= 63 else "logmel")
        for hist in [h for h in M.HISTS if h >= n]:
            for wrap in (False, True):
                # (a wrapping span starts (n + 1) // 2 slots before the ring's end -- for n = 1 in its last slot)
                first = 2 * hist + (hist - (n + 1) // 2 if wrap else min(3, hist - n))
                end = first + n + min(1, hist - n)
                for width in M.widths_of(n):
                    k = len(jobs)
                    dtype, normalize = (F16 if k % 2 else F32), (RAW if k % 3 == 2 else PER_FEATURE)
                    ld = width + (0, 1, 5)[k % 3]
                    off = (0, 1, 3)[k % 3]           # (float16: odd element offsets; float32: offsets that are 4-byte aligned only)
                    jobs.append(_job(values, hist, first, end, width, normalize, dtype, (0.0, -2.5, 1.0)[k % 3], ld, off))
                    vals.append(values)
    assert 4 <= len(jobs) <= 64
    assert any((j["first_frame"] % j["hist"]) + n > j["hist"] for j in jobs) or n == 1
    for j, v, got in zip(jobs, vals, handle.nemo_chunk_kernel(jobs)):
        _check(j, got, v, (n, j["n_mels"], j["hist"], j["first_frame"] % j["hist"], j["width"], j["dtype"], j["normalize"]))


@pytest.mark.parametrize("hist,n", ((32, 20), (33, 33), (3000, 129)))
def test_every_ring_phase_gives_the_same_bits(handle, hist, n):
    """one fixed set of values as a span that starts in every slot 0 .. hist - 1 of the ring: mean, std and output are the model's,
    hence identical bits across the phases"""
    values = M.frames(80, n, 77, "mixed")
    width = n + 3
    want, mean, std = (M.bits(a).reshape(-1) for a in M.chunk(values, width, True))
    seen = 0
    for p0 in range(0, hist, 64):
        phases = list(range(p0, min(p0 + 64, hist)))
        jobs = [_job(values, hist, hist + p, hist + p + n + min(2, hist - n), width, PER_FEATURE, F32) for p in phases]
        for p, j, got in zip(phases, jobs, handle.nemo_chunk_kernel(jobs)):
            assert j["first_frame"] % hist == p
            if p % 64 == 0:
                _check(j, got, values, (hist, "phase", p))
            out = M.bits(got["out"])
            assert np.array_equal(out[:80 * width], want) and (out[80 * width:] == M.CANARY).all(), (hist, "phase", p)
            assert np.array_equal(M.bits(got["mean"]), mean) and np.array_equal(M.bits(got["std"]), std), (hist, "phase", p)
            seen += 1
    assert seen == hist


def test_tables_of_1_32_and_33(handle):
    """mixed modes, dtypes, band counts and widths in one call: every item is the model's, and equals the same item alone"""
    jobs, vals = [], []
    for k in range(33):
        n_mels, n = (128 if k % 4 == 1 else 80), (1, 7, 64, 65, 200)[k % 5]
        hist = (32 if n <= 32 else 256) + k % 2
        values = M.frames(n_mels, n, 300 + k)
        first = hist + (hist - n // 2 - 1 if k % 3 == 0 else k)
        jobs.append(_job(values, hist, first, first + n, n + k % 4, PER_FEATURE if k % 2 else RAW, F16 if k % 3 == 1 else F32, 0.5 * (k % 3), n + k % 4 + k % 2, k % 3))
        vals.append(values)
    fresh = lambda j: dict(j, out=j["out"].copy(), mean=j["mean"].copy(), std=j["std"].copy())
    alone = [handle.nemo_chunk_kernel([fresh(j)])[0] for j in jobs]
    for count in (1, 32, 33):
        for j, v, got, one in zip(jobs[:count], vals, handle.nemo_chunk_kernel([fresh(j) for j in jobs[:count]]), alone):
            _check(j, got, v, ("table of", count))
            for name in ("out", "mean", "std"):
                assert np.array_equal(_words(got[name]), _words(one[name])), (count, name)


def test_refusals_leave_everything_untouched(handle):
    L = pkg("_lib")
    values = M.frames(80, 40, 9)
    good = lambda **kw: dict(_job(values, 64, 100, 150, 48, PER_FEATURE, F32, 0.0, 50, 2), **kw)
    handle.nemo_chunk_kernel([good()])
    short = lambda name, by=1: {name: good()[name][:-by]}
    bad = [dict(n_mels=64), dict(dtype=2), dict(dtype=-1), dict(normalize=2), dict(normalize=-1), dict(n_frames=0), dict(n_frames=49),
           dict(width=39), dict(width=3001, ld=3001), dict(ld=47), dict(pad_value=float("inf")), dict(pad_value=float("nan")),
           dict(hist=0), dict(first_frame=85), dict(first_frame=111), dict(first_frame=-1), dict(end_frame=-1), dict(out_offset=-1),
           dict(hist=32), short("ring"), short("out", SLACK + 3), short("mean"), short("std"), dict(ring=None), dict(out=None)]
    for kw in bad:
        jobs = [good(), good(**kw)]
        before = [{k: v.copy() for k, v in j.items() if isinstance(v, np.ndarray)} for j in jobs]
        with pytest.raises(L.CssError) as e:
            handle.nemo_chunk_kernel(jobs)
        assert e.value.code == L.CSS_ERR_INVALID_ARG and "css_nemo_chunk_host" in str(e.value), (kw, str(e.value))
        for j, b, left in zip(jobs, before, e.value.left):
            for k, v in b.items():
                assert np.array_equal(_words(j[k]), _words(v)), (kw, "the caller's", k)
                if k in left:
                    assert np.array_equal(_words(left[k]).reshape(-1), _words(v).reshape(-1)), (kw, k, "as the call left it")
    for count in (0, 65):
        with pytest.raises(L.CssError) as e:
            handle.nemo_chunk_kernel([good() for _ in range(count)])
        assert e.value.code == L.CSS_ERR_INVALID_ARG


# ---- the ring write of the mel kernel -------------------------------------------------------------------------------------------------

def _spectra(ld, seed):
    """[514][ld] float32: per column a level between 1e-6 and 10 (quiet columns reach the guard), rows of mixed sign"""
    rng = np.random.default_rng(seed)
    level = 10.0 ** rng.uniform(-6, 1, ld)
    spec = (rng.standard_normal((514, ld)) * level[None, :]).astype(np.float32)
    spec[:, ::7] = 0
    return spec


@pytest.mark.parametrize("hist", (32, 64))
def test_mel_with_a_history(handle, hist):
    """rounds of 1, 31, 32, 33 and 150 frames (and none) per speaker, from frame counts that make the round wrap: mel is the plain
    entry's bit for bit, the ring is the model's whole -- slots the round does not own keep their canaries"""
    S, rounds = 3, (1, 31, 32, 33, 150, 0, 33, 150, 31)
    jobs, row0 = [], 2
    for i in range(len(rounds) // S * S // S):
        n_new = np.array(rounds[S * i:S * i + S], np.int32)
        rows = int(max(n_new.max(), 1)) + i
        nm = 128 if i == 1 else 80
        J0 = np.array([0, hist - 1, 5 * hist + hist // 2], np.int64) + i        # (a first round; one that wraps; one in the middle)
        jobs.append(dict(n_mels=nm, row0=row0, rows=rows, mel_ld=rows + 3, hist=hist, n_new=n_new, frames_after=J0 + n_new,
                         mel=M.canary(S * nm * (rows + 3) + SLACK), ring=M.canary(S * nm * hist + SLACK)))
        row0 += S * rows + 1
    ld = row0 + 4
    spec = _spectra(ld, 60 + hist)
    plain = handle.stream_nemo_mel(S, spec, ld, [{k: v for k, v in j.items() if k not in ("hist", "ring", "frames_after")} for j in jobs])
    together = handle.stream_nemo_mel_history(S, spec, ld, jobs)
    seen = set()
    for i, (job, got, ref) in enumerate(zip(jobs, together, plain)):
        nm, mel_ld = job["n_mels"], job["mel_ld"]
        assert np.array_equal(M.bits(got["mel"]), M.bits(ref["mel"])), f"job {i}: mel against the entry without a history"
        mel = got["mel"][:S * nm * mel_ld].reshape(S, nm, mel_ld)
        ring = got["ring"][:S * nm * hist].reshape(S, nm, hist)
        assert (M.bits(got["ring"][S * nm * hist:]) == M.CANARY).all(), f"job {i}: behind the ring"
        for k in range(S):
            n_new = int(job["n_new"][k])
            J0 = int(job["frames_after"][k]) - n_new
            want = M.ring_after_round(np.tile(M.canary(hist), (nm, 1)), J0, mel[k, :, :n_new])
            assert np.array_equal(M.bits(ring[k]), M.bits(want)), (i, k, n_new, J0)
            assert int((M.bits(ring[k][0]) != M.CANARY).sum()) == min(n_new, hist)
            seen.add(n_new)
        (alone,) = handle.stream_nemo_mel_history(S, spec, ld, [dict(job, mel=M.canary(job["mel"].size), ring=M.canary(job["ring"].size))])
        assert np.array_equal(M.bits(alone["ring"]), M.bits(got["ring"])) and np.array_equal(M.bits(alone["mel"]), M.bits(got["mel"]))
    assert seen == set(rounds)


def test_mel_history_refusals(handle):
    L = pkg("_lib")
    S, hist, nm, rows = 3, 32, 80, 40
    ld = S * rows + 8
    spec = _spectra(ld, 5)
    good = lambda **kw: dict(dict(n_mels=nm, row0=1, rows=rows, mel_ld=rows, hist=hist, n_new=np.array([3, 0, 40], np.int32),
                                  frames_after=np.array([3, 7, 400], np.int64), mel=M.canary(S * nm * rows), ring=M.canary(S * nm * hist)), **kw)
    handle.stream_nemo_mel_history(S, spec, ld, [good()])
    for kw in (dict(hist=0), dict(frames_after=np.array([2, 7, 400], np.int64)), dict(frames_after=np.array([3, 7], np.int64)),
               dict(ring=M.canary(S * nm * hist - 1)), dict(ring=None), dict(frames_after=None), dict(n_mels=64), dict(rows=0), dict(mel_ld=rows - 1)):
        jobs = [good(), good(**kw)]
        with pytest.raises(L.CssError) as e:
            handle.stream_nemo_mel_history(S, spec, ld, jobs)
        assert e.value.code == L.CSS_ERR_INVALID_ARG and "css_stream_nemo_mel_history_host" in str(e.value), (kw, str(e.value))
        for left in e.value.left:
            assert all((M.bits(v) == M.CANARY).all() for v in left.values()), kw
