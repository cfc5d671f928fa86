"""tests/stream_nemo_reference.py on the CPU: rounds of the model of the streamed NeMo append compose, over every cutting, to the
operand rows and the ranges of the whole recording's definition (tests/nemo_reference.py, tests/handoff_reference.py) and to
``stream.nemo_features``; the cases the format adds are what their names say; every named mistake breaks the case listed for it."""
import numpy as np
import pytest

import nemo_reference as N
import stream_nemo_reference as M
from conftest import pkg

CASES = M.cases() + M.random_cases()
BY_NAME = {c["name"]: c for c in CASES}


def _agrees(c, got):
    """the chain's result against the definition, speaker by speaker -> the list of what differs"""
    bad = []
    for k in range(c["S"]):
        ranges, fr, x = M.definition(c, k)
        rows, rg, A, J = got[k]
        if not np.array_equal(rg, ranges):
            bad.append((k, "ranges"))
        if A != len(x) or J != len(fr) or J != len(x) // 160:
            bad.append((k, "counts", A, len(x), J, len(fr)))
        elif not np.array_equal(M.bits(rows), M.bits(fr)):
            bad.append((k, "operand rows"))
    return bad


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_rounds_compose_to_the_whole_recording(c):
    assert _agrees(c, M.chain(c)) == []


def test_the_cases_are_what_they_are_named_for():
    assert len(BY_NAME) == len(CASES)
    assert {c["pad"] for c in CASES if c["name"].startswith("random")} == {0, 3, 8}
    assert {c["drop"] for c in CASES if c["name"].startswith("random")} == {0, 1}

    def states(name):
        """per round: (round, [A before, A after] of speaker 0, ranges speaker 0 appended)"""
        c, out, state = BY_NAME[name], [], M.state0(BY_NAME[name])
        for rnd in M.rounds_of(c):
            job = M.job_of(c, rnd, state)
            res = [M.append_round(job, k) for k in range(c["S"])]
            out.append((rnd, int(job["st"][0]["A"]), res[0]["A1"], res[0]["ranges"], [r["n_new"] for r in res]))
            state = M.next_state(job, res)
        return out, state

    # a seam exactly on a round boundary: a round whose first kept sample starts a new range at its own D0, with samples before it
    rounds, _ = states("seam_on_round_boundary")
    assert any(A0 > 0 and rg and rg[0][0] == rnd[2] and prev_end < rnd[2]
               for (rnd, A0, _, rg, _), prev_end in zip(rounds[1:], [max([r[3][-1][1]] if r[3] else [0]) for r in rounds[:-1]]))
    # a round that appends nothing: with t_g unmoved, and inside a pause
    rounds, _ = states("round_appends_nothing")
    assert any(rnd[0] == rnd[1] for rnd, *_ in rounds) and any(rnd[1] > rnd[0] and A1 == A0 for rnd, A0, A1, _, _ in rounds)
    # A crosses 256 inside a round, and further samples follow in that round
    rounds, _ = states("A_crosses_256_in_round")
    assert any(A0 < 256 < A1 for _, A0, A1, _, _ in rounds)
    # no frame ever; frames at finish only
    rounds, state = states("A_below_160")
    assert 0 < int(state[2][0]["A"]) < 160 and all(n == [0, 0, 0] for *_, n in rounds)
    rounds, state = states("A_160_to_256")
    assert 160 <= int(state[2][0]["A"]) < 256 and all(n == [0, 0, 0] for *_, n in rounds[:-1]) and rounds[-1][4] == [1, 0, 1]
    # a speaker never active
    for name in ("seam_on_round_boundary", "pad3_seams"):
        _, state = states(name)
        assert int(state[2][1]["A"]) == 0 and int(state[2][1]["J"]) == 0
    # rounds of more than 256 blocks are among stream_reference's cases
    assert any((D1 - D0) // 256 > 256 for c in CASES for _, _, D0, D1, _ in M.rounds_of(c))


@pytest.mark.parametrize("mut", M.MISTAKES)
def test_named_mistakes_break_their_case(mut):
    c = BY_NAME[M.CAUGHT_BY[mut]]
    assert _agrees(c, M.chain(c)) == []
    assert _agrees(c, M.chain(c, mut)) != [], (mut, c["name"])


def test_model_rows_give_nemo_features():
    """the frames the rounds emitted, through the package's numpy statement of the features, are ``nemo_features`` of the kept
    samples (the same arrays through the same numpy calls: equal bits)"""
    S = pkg("stream")
    c = BY_NAME["pad3_seams"]
    got = M.chain(c)
    checked = 0
    for k in range(c["S"]):
        rows, _, A, J = got[k]
        _, _, x = M.definition(c, k)
        want = S.nemo_features(x, 80, c["preemphasis"], normalize=False)
        assert want.shape == (80, J)
        if J == 0:
            continue
        # the padded signal the emitted rows spell out (row j is its floats [160 j, 160 j + 512): the overlaps must agree), then
        # nemo_features' own lines on it, so that numpy multiplies arrays of the same layout
        padded = np.zeros(160 * (J - 1) + 512, np.float32)
        for j in range(J):
            assert j == 0 or np.array_equal(M.bits(padded[160 * j:160 * j + 352]), M.bits(rows[j][:352]))
            padded[160 * j:160 * j + 512] = rows[j]
        Am, W = S.nemo_tables(80)
        frames = np.lib.stride_tricks.sliding_window_view(padded, 512)[::160][:J].T
        spec = Am @ frames
        power = spec[:257] * spec[:257] + spec[257:] * spec[257:]
        raw = np.log((W @ power).astype(np.float32) + np.float32(2.0 ** -24)).astype(np.float32)
        assert np.array_equal(raw, want), k
        checked += 1
    assert checked >= 2


def test_frame_rule_and_rows():
    for A in range(0, 2000):
        J = M.open_frames(A)
        assert (J == 0 and A < 256) or (160 * (J - 1) + 256 <= A < 160 * J + 256)
        assert J <= A // 160 and A - (160 * J - 256) < M.TAIL_LD
        assert A - (160 * (A // 160) - 256) < M.TAIL_LD
    for dn in (0, 1, 159, 160, 255, 256, 257, 4000, 70000):
        for A0 in (0, 100, 255, 256, 300, 415, 416, 1000):
            J0 = M.open_frames(A0)
            # every new sample has its column, and a closing round's last frame its 512 columns, inside the speaker's rows
            assert A0 + dn - (160 * J0 - 256) <= M.nemo_rows(dn) * 160
            assert ((A0 + dn) // 160 - J0 - 1) * 160 + 512 <= M.nemo_rows(dn) * 160
