"""tests/handoff_reference.py on the CPU: the float64 reference of the Whisper log-mel hand-off against the oracle's numpy
restatement and against the committed vectors of the published definition; a float32 restatement of the device path inside the
bound on every signal and gate of the GPU test's own list; every named mistake above the bound on a case of that list; and the
bound small enough beside the mistakes.  DESIGN.md 7 N4 ("The hand-off's values") has the count table."""
import os

import numpy as np
import pytest

import css_oracle as O
import handoff_reference as H

from conftest import GOLDEN

TL, N_OUT = 374, 96000           # the pass of tests/test_hip_handoff_values.py: 6 s, (TL + 1) 256 samples per stream
CASES = {c["name"]: c for c in H.cases(TL)}


def _case(name, row):
    """(ranges, waveform row, concatenation, reference) of one stream row of a case (computed once, shared with the GPU module)"""
    return H.case_reference(CASES[name], row, TL, N_OUT)[1:]


def _mistaken(name, row, mut):
    ranges, w, _, _ = _case(name, row)
    return H.reference(H.concat(w, ranges, mut), CASES[name]["n_mels"], mut, want_bound=False)


# ---- the reference is the definition ------------------------------------------------------------------------------------------

def test_kept_ranges_are_the_oracles():
    rs = np.random.RandomState(3)
    for pad in (0, 1, 8):
        for density in (0.02, 0.2, 0.9):
            g = (rs.rand(TL) < density).astype(np.uint8)
            assert np.array_equal(H.kept_ranges(g, pad, N_OUT), O.active_regions(g.astype(bool), pad, N_OUT))
    assert np.array_equal(H.kept_ranges(np.zeros(TL, np.uint8), 8, N_OUT, drop=False), [[0, N_OUT]])
    for blocks, frames in ((2, 3), (19, 30), (20, 32), (21, 33), (22, 35), (40, 64), (41, 65)):
        r = H.kept_ranges(H.gate_of(TL, [(60, blocks)]), 0, N_OUT)
        assert r.tolist() == [[60 * 256, (60 + blocks) * 256]] and H.frames_of(blocks * 256) == frames
        assert (blocks * 256 % 160 < 40) == (blocks % 5 in (0, 2))       # the counts that read the right-hand reflection


@pytest.mark.parametrize("n_mels", (80, 128))
def test_reference_against_the_oracle(n_mels):
    worst = 0.0
    for kind, n in (("noise", 16000), ("tones", 4777), ("chirp", N_OUT), ("quiet_chirp_3e-2", N_OUT), ("square", 5120), ("zeros", 800)):
        x = H.signal(kind, n)
        ref = H.reference(x, n_mels)
        got = O.whisper_log_mel(x, n_mels)
        assert got.shape == ref.out.shape == (n_mels, n // 160)
        q = np.abs(got - ref.out) / H.oracle_tolerance(ref)
        assert q.max() <= 1.0, (kind, float(q.max()), np.unravel_index(int(q.argmax()), q.shape))
        worst = max(worst, float(q.max()))
    print(f"reference against the oracle, n_mels {n_mels}: worst ratio {worst:.3f}")
    assert H.reference(np.zeros(159, np.float32), n_mels).out.shape == (n_mels, 0)


@pytest.mark.parametrize("n_mels", (80, 128))
def test_reference_against_the_committed_vectors(n_mels):
    """torch.stft in float32 and a float32 filterbank product round less often than the device path's 400-term chains, so the
    vectors lie inside the device bound of the reference; the filterbank itself is one rounding from the formula"""
    g = np.load(os.path.join(GOLDEN, "whisper_logmel_r5.npz"))
    bank = g[f"mel_filters_{n_mels}"]
    W = H.mel_bank(n_mels)
    assert bank.shape == W.shape and (np.abs(bank - W) <= H.U * np.abs(W) * H.SECOND + 1e-17).all()
    assert (np.abs(O._slaney_mel_bank(n_mels) - W) <= H.U * np.abs(W) * H.SECOND + 1e-17).all()
    x = (0.1 * np.random.RandomState(5).randn(7 * 16000)).astype(np.float32)          # gen_golden_whisper.py's "clip7"
    ref = H.reference(x, n_mels)
    vec = g[f"clip7_logmel_{n_mels}"]
    assert vec.shape == ref.out[:, ::3].shape
    q = np.abs(vec - ref.out[:, ::3]) / ref.bound[:, ::3]
    print(f"reference against the committed vectors, n_mels {n_mels}: worst ratio {q.max():.3f}")
    assert q.max() <= 1.0


def test_tables_are_the_stated_ones():
    A = H.analysis_matrix()
    w = H.hann()
    assert w[0] == 0 and w[200] == 1 and np.array_equal(w[1:], w[:0:-1])               # periodic: w[n] == w[400 - n]
    assert not np.array_equal(H.hann("symmetric_hann")[1:], H.hann("symmetric_hann")[:0:-1])
    x = np.random.default_rng(0).standard_normal(400)
    spec = np.fft.rfft(x * w)
    assert np.allclose(A[:201] @ x, spec.real, atol=1e-11) and np.allclose(A[201:] @ x, spec.imag, atol=1e-11)
    op = H.operand(np.arange(1000.0))
    assert np.array_equal(op, np.pad(np.arange(1000.0), 200, mode="reflect"))
    assert np.array_equal(H.operand(np.arange(1000.0), "left_edge_repeat")[:200], np.pad(np.arange(1000.0), 200, mode="symmetric")[:200])
    assert np.array_equal(H.operand(np.arange(1000.0), "right_edge_repeat")[-200:], np.pad(np.arange(1000.0), 200, mode="symmetric")[-200:])


def test_case_list_covers_what_the_issue_names():
    names = list(CASES)
    for blocks in (2, 19, 20, 21, 22, 40, 41):
        assert f"{blocks}_blocks" in names
    met = {}
    for c in CASES.values():
        assert "impulses" in c["kinds"] or not c["drop"]
        for row in range(3):
            _, ranges, w = H.case_row(c, row, TL, N_OUT)
            assert w.shape == (N_OUT,) and w.dtype == np.float32 and ranges[-1, 1] <= N_OUT
            met.setdefault(c["kinds"][row], set()).add((c["n_mels"], len(ranges)))
    for kind in H.SIGNALS:
        assert {nm for nm, _ in met[kind]} == {80, 128}, kind
    assert {nr for _, nr in met["impulses"]} >= {1, 2, 3} and {nr for _, nr in met["chirp"]} >= {1, 2, 3}
    assert {c["ld_extra"] for c in CASES.values()} == {0, 1} and any(c["pad"] == 8 and c["drop"] for c in CASES.values())
    # the quiet signals are what the issue asks of them: every log negative and the floor reached on both; the clamp below the
    # floor at 3e-3 (the floor decides, -1.5 bit for bit), above it at 3e-2 (the clamp decides: what the mistakes of the maximum need)
    lo, hi = _case("whole_128", 2)[3], _case("whole_80_b", 0)[3]
    assert lo.raw.max() < 0 and lo.mx - 8 < -10 and lo.exact.mean() > 0.5
    assert hi.raw.max() < 0 and hi.mx - 8 > -10 and (hi.mel <= H.FLOOR).any() and hi.clamped.mean() > 0.5 and not hi.exact.any()
    ch = _case("whole_80", 1)[3]
    assert ch.raw.max() > 0 and ch.clamped[:, :100].mean() > 0.9                         # the clamp decides the chirp's early frames


# ---- the device path in float32 stays inside the bound --------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_float32_model_inside_the_bound(name):
    c = CASES[name]
    for row in range(3):
        _, _, x, ref = _case(name, row)
        got = H.model32(x, c["n_mels"])
        assert got.shape == ref.out.shape and got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - ref.out)
        q = np.where(err == 0, 0.0, err / ref.bound)
        pos = np.unravel_index(int(q.argmax()), q.shape)
        print(f"{name} row {row} {c['kinds'][row]} n_mels {c['n_mels']}: float32 model worst ratio {q[pos]:.4f} at {pos}")
        assert q[pos] <= 1.0, (name, row, float(q[pos]), pos)
        assert (H.bits(got[ref.exact]) == H.bits(np.float32(-1.5))).all(), (name, row, "an element at the floor is not -1.5")
        cl = H.bits(got[ref.clamped])
        assert cl.size == 0 or (cl == cl[0]).all(), (name, row, "surely clamped elements differ")
        if c["kinds"][row] == "zeros":
            assert ref.exact.all()


# ---- every named mistake exceeds the bound on a case of the list ----------------------------------------------------------------

@pytest.mark.parametrize("mut", H.MISTAKES)
def test_mistake_exceeds_the_bound(mut):
    assert H.CAUGHT_BY[mut]
    for name, row in H.CAUGHT_BY[mut]:
        ref = _case(name, row)[3]
        q, pos = H.deviation(_mistaken(name, row, mut), ref)
        print(f"{mut}: {name} row {row} ({CASES[name]['kinds'][row]}): deviation / bound {q:.3g} at {pos}")
        assert q > 1.0, (mut, name, row, q)


def test_issue_named_signals_catch_their_mistakes():
    """the operand roundings on the two tones; the maximum's mistakes and the misplaced floor on the quiet chirp whose clamp lies
    above the floor; the reflections and the seam on the impulses"""
    kinds = lambda mut: {CASES[n]["kinds"][r] for n, r in H.CAUGHT_BY[mut]}
    assert "tones" in kinds("bf16_operands") and "tones" in kinds("f16_operands")
    for mut in ("tile_max", "signed_bits_max", "floor_after_log"):
        assert "quiet_chirp_3e-2" in kinds(mut)
    assert "quiet_chirp" in kinds("floor_after_log")
    for mut in ("left_edge_repeat", "right_edge_repeat", "offs_plus_one"):
        assert "impulses" in kinds(mut)
    assert set(H.CAUGHT_BY) == set(H.MISTAKES) and len(H.MISTAKES) == 12


def test_right_reflection_is_read_only_by_the_stated_block_counts():
    for name, row in H.RIGHT_REFLECTION_UNREAD:
        x, ref = _case(name, row)[2:]
        assert len(x) % 160 >= 40
        assert H.deviation(_mistaken(name, row, "right_edge_repeat"), ref)[0] == 0.0
    for name, row in H.CAUGHT_BY["right_edge_repeat"]:
        assert len(_case(name, row)[2]) % 160 < 40


def test_bound_is_small_beside_the_mistakes():
    """per signal family: the share of well-conditioned elements (bound <= COND) and the worst bound among them, which is at most
    COND; and every mistake moves a well-conditioned element of its first case by more than ten times COND.  (Elements that are
    not well conditioned hold leakage at the level of the product's absolute error, 401 U sum |a x|, next to the clamp threshold:
    most of the square wave's, a few per cent elsewhere.)"""
    share, worst = {}, {}
    for c in CASES.values():
        for row in range(3):
            ref = _case(c["name"], row)[3]
            kind = c["kinds"][row]
            good = ref.bound <= H.COND
            share.setdefault(kind, []).append(good.reshape(-1))
            worst[kind] = max(worst.get(kind, 0.0), float(ref.bound[good].max()) if good.any() else 0.0)
    for kind in H.SIGNALS:
        s = float(np.concatenate(share[kind]).mean())
        print(f"{kind}: {100 * s:.1f} % of the elements well conditioned, worst bound among them {worst[kind]:.3g}")
        assert s >= (0.3 if kind == "square" else 0.9), (kind, s)
    smallest = np.inf
    for mut in H.MISTAKES:
        name, row = H.CAUGHT_BY[mut][0]
        ref, m = _case(name, row)[3], _mistaken(name, row, mut)
        if m.out.shape != ref.out.shape:
            continue                                         # (a frame count: no value to compare)
        d = float(np.abs(m.out - ref.out)[ref.bound <= H.COND].max())
        print(f"{mut}: moves a well-conditioned element of {name} row {row} by {d:.3g}")
        smallest = min(smallest, d)
    assert smallest > 10 * H.COND >= 10 * max(worst.values()), smallest
