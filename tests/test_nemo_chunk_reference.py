"""tests/nemo_chunk_reference.py on the CPU: the exact model of a NeMo chunk and of the ring after a round.  The model's statistics
lie within the derived bound of numpy's float64 two-pass values, the package's numpy statement (stream.py nemo_chunk_features) is
the model bit for bit, a chunk over all frames of a stream is nemo_features(normalize=True) within tests/nemo_reference.py's
bound, and every named mistake breaks a listed case."""
import numpy as np
import pytest

import nemo_chunk_reference as M
import nemo_reference as N
from conftest import pkg

CASES = M.cases()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_statistics_lie_within_the_derived_bound(case):
    _, n_mels, n, kind, seed = case
    raw = M.frames(n_mels, n, seed, kind)
    mean, std = M.stats(raw)
    ref_mean, ref_std = M.reference_stats(raw)
    max_abs = float(np.abs(raw).max())
    e_mean, e_std = np.abs(mean.astype(np.float64) - ref_mean), np.abs(std.astype(np.float64) - ref_std)
    b_mean, b_std = M.stats_bound(ref_mean, n, max_abs), M.stats_bound(ref_std, n, max_abs)
    print(case[0], "mean error / bound", float((e_mean / b_mean).max()), "std error / bound", float((e_std / b_std).max()))
    assert (e_mean <= b_mean).all() and (e_std <= b_std).all()
    assert mean.dtype == np.float32 and std.dtype == np.float32 and np.isfinite(mean).all() and np.isfinite(std).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_the_packages_numpy_statement_is_the_model(case):
    S = pkg("stream")
    _, n_mels, n, kind, seed = case
    raw = M.frames(n_mels, n, seed, kind)
    mean, std = S.nemo_chunk_stats(raw)
    m_mean, m_std = M.stats(raw)
    assert _same_bits(mean, m_mean) and _same_bits(std, m_std)
    for width in M.widths_of(n):
        for normalize, dtype, pad in (("per_feature", "float32", 0.0), ("per_feature", "float16", -1.5), (None, "float32", 0.25), (None, "float16", 0.0)):
            out, _, _ = M.chunk(raw, width, normalize is not None, np.dtype(dtype), pad)
            assert _same_bits(S.nemo_chunk_features(raw, width, normalize, dtype, pad), out), (case[0], width, normalize, dtype)
    assert _same_bits(S.nemo_chunk_features(raw), M.chunk(raw)[0])     # (the defaults: width = n, per feature, float32, pad 0)


def test_the_statement_refuses_what_the_call_refuses():
    S = pkg("stream")
    raw = M.frames(80, 10)
    for kw in (dict(width=9), dict(width=3001), dict(dtype="bfloat16" if hasattr(np, "bfloat16") else "float64"), dict(normalize="all_features"),
               dict(pad_value=float("inf")), dict(pad_value=float("nan"))):
        with pytest.raises(ValueError):
            S.nemo_chunk_features(raw, **kw)
    with pytest.raises(ValueError):
        S.nemo_chunk_features(raw[:, :0])
    with pytest.raises(ValueError):
        S.nemo_chunk_stats(raw[0])


def test_a_chunk_over_all_frames_is_the_sessions_normalisation():
    """width == n over every frame of a stream: within the bound tests/nemo_reference.py states for the session call's output"""
    S = pkg("stream")
    for kind, n_mels, seconds in (("speechlike", 80, 2.0), ("noise", 128, 1.0), ("quiet", 80, 1.5)):
        x = N.signal(kind, int(16000 * seconds), 5)
        raw = S.nemo_features(x, n_mels, 0.97, normalize=False)
        ref = N.reference(x, [[0, len(x)]], n_mels, 0.97, normalize=True)
        out, mean, std = M.chunk(raw, raw.shape[1], True)
        assert out.shape == ref.out.shape and raw.shape[1] == len(x) // 160 > 1
        err = np.abs(out.astype(np.float64) - ref.out)
        print(kind, "largest error / bound", float((err / ref.bound).max()))
        assert (err <= ref.bound).all()
        assert (np.abs(mean - ref.mean) <= ref.e_mean).all() and (np.abs(std - ref.std) <= ref.e_std).all()
        # ... and nemo_features' own normalisation of the same frames within the same bound
        assert (np.abs(S.nemo_features(x, n_mels, 0.97, normalize=True).astype(np.float64) - ref.out) <= ref.bound).all()


def test_a_constant_band_has_zero_std_and_finite_outputs():
    for n in (1, 2, 64, 200, 3000):
        raw = M.frames(80, n, kind="silence")
        out, mean, std = M.chunk(raw, min(n + 7, M.MAX_WIDTH), True, np.float32, 0.0)
        assert (std == 0.0).all() and (mean == M.SILENCE).all() and np.isfinite(out).all() and (out == 0.0).all()
    raw = M.frames(128, 300, 3, "mixed")
    for dtype in (np.float32, np.float16):
        out, mean, std = M.chunk(raw, 300, True, dtype)
        assert std[64] == 0.0 and (std[:64] > 0).all() and np.isfinite(out.astype(np.float32)).all() and (out[64] == 0).all()


# ---- the named mistakes ---------------------------------------------------------------------------------------------------------------

def _broken(mut):
    """a listed case the mistake breaks: (the definition's result, the mistaken one) as tuples of arrays"""
    if mut in ("biased", "eps_inside"):
        raw = M.frames(80, 65, 4)
        return M.chunk(raw, 66, True), M.chunk(raw, 66, True, mut=mut)
    if mut in ("stats_over_width", "pad_normalised"):
        raw = M.frames(80, 127, 5)
        return M.chunk(raw, 128, True, pad_value=0.0), M.chunk(raw, 128, True, pad_value=0.0, mut=mut)
    if mut == "n1_nan":
        raw = M.frames(80, 1, 0)
        return M.chunk(raw, 2, True), M.chunk(raw, 2, True, mut=mut)
    if mut == "float32_stats":
        raw = M.frames(128, 3000, 10)
        return M.chunk(raw, 3000, True), M.chunk(raw, 3000, True, mut=mut)
    rounds = {"slot_plus_one": (32, 5, 31), "oldest_last": (32, 40, 150)}[mut]      # (hist, J0, n_new)
    hist, J0, n_new = rounds
    fr = M.frames(80, J0 + n_new, 6)
    ring = M.ring_holding(fr, hist, J0)
    return (M.ring_after_round(ring, J0, fr[:, J0:]),), (M.ring_after_round(ring, J0, fr[:, J0:], mut=mut),)


@pytest.mark.parametrize("mut", M.MISTAKES)
def test_every_named_mistake_breaks_a_listed_case(mut):
    good, bad = _broken(mut)
    differs = [not np.array_equal(g, b, equal_nan=True) for g, b in zip(good, bad) if g is not None]
    assert any(differs), mut
    if mut == "n1_nan":
        assert np.isnan(bad[0][:, 0]).all() and np.isfinite(good[0]).all() and (good[2] == 0).all()
    if mut == "pad_normalised":
        assert (good[0][:, 127] == 0.0).all() and (bad[0][:, 127] != 0.0).all()
    if mut == "float32_stats":   # beyond the derived bound for at least one band, not just other bits
        raw = M.frames(128, 3000, 10)
        ref_mean, ref_std = M.reference_stats(raw)
        mx = float(np.abs(raw).max())
        over = (np.abs(bad[1] - ref_mean) > M.stats_bound(ref_mean, 3000, mx)) | (np.abs(bad[2] - ref_std) > M.stats_bound(ref_std, 3000, mx))
        assert over.any()


def test_the_ring_after_any_chain_of_rounds_holds_the_last_frames():
    """rounds of 1, 31, 32, 33 and 150 frames into rings of 32 and 64, from counts that wrap: after every round the ring holds
    [max(J - hist, 0), J), and a span of it is the frames' own columns whatever slot it starts in"""
    for hist in (32, 64):
        fr = M.frames(80, 600, hist)
        ring, J = np.tile(M.canary(hist), (80, 1)), 0
        for n_new in (1, 31, 32, 33, 150, 1, 33, 150, 31):
            ring = M.ring_after_round(ring, J, fr[:, J:J + n_new])
            J += n_new
            first = max(J - hist, 0)
            assert np.array_equal(M.bits(M.span(ring, first, J - first)), M.bits(fr[:, first:J]))
            assert np.array_equal(M.bits(ring), M.bits(M.ring_holding(fr, hist, J)))
        assert J == 462
