"""The kernels of csrc/nemo.hip on the MI355X through Handle.nemo_kernels (css_nemo_kernels_host): gather, the exact float32
product, mel, statistics and normalisation as the path launches them, on caller rows and run tables.  The frame operand is held
to its exact model bit for bit; the raw ln rows, mean, std and the normalised rows to the counted bound of
tests/nemo_reference.py -- every element, none left out --; every output is returned whole and must hold its canary wherever the
launches do not write."""
import numpy as np
import pytest

import nemo_reference as N
from conftest import pkg
from test_hip_window_kernels import _open, _same_bits

pytestmark = pytest.mark.gpu

CAN = N.CANARY


@pytest.fixture(scope="module")
def handle():
    sep = _open()
    yield sep.handle
    sep.close()


def _run(handle, streams, n_mels, p, normalize, wav_off=0, extra_rows=0, out_extra=5):
    """streams: [(row float32, ranges [n][2])] -> (job outputs reshaped, geometry).  Every output starts as canaries."""
    L = pkg("_lib")
    S = len(streams)
    cap = max(max(len(np.asarray(r).reshape(-1, 2)) for _, r in streams), 1) + 1
    wav_ld = max(len(row) for row, _ in streams) + 3
    wav = np.full(wav_off + S * wav_ld, 1e30, np.float32)               # (what lies outside the ranges must not matter)
    regs, offs = np.zeros((S, cap, 2), np.int64), np.zeros((S, cap), np.int64)
    st, nr = np.zeros(S, L.HANDOFF_STATE), np.zeros(S, np.int32)
    for k, (row, ranges) in enumerate(streams):
        wav[wav_off + k * wav_ld:wav_off + k * wav_ld + len(row)] = row
        regs[k], offs[k], A, nr[k] = N.run_table(ranges, cap)
        st[k]["A"], st[k]["J"] = A, A // 160
    rows = int(st["J"].max()) + 4 + extra_rows
    raw_ld, out_ld = rows - 4 + 3, int(st["J"].max()) + out_extra
    job = dict(S=S, n_mels=n_mels, normalize=int(normalize), cap_ranges=cap, wav_off=wav_off, preemphasis=p, wav_ld=wav_ld, rows=rows,
               raw_ld=raw_ld, out_ld=out_ld, wav=wav, regs=regs, offs=offs, st=st, n_ranges=nr,
               operand=N.canary(S * rows * 160 + 512), raw=N.canary(S * n_mels * raw_ld), mean=N.canary(S * n_mels),
               stdv=N.canary(S * n_mels), out=N.canary(S * n_mels * out_ld))
    got = handle.nemo_kernels(job)
    return dict(operand=got["operand"], raw=got["raw"].reshape(S, n_mels, raw_ld), mean=got["mean"].reshape(S, n_mels),
                std=got["stdv"].reshape(S, n_mels), out=got["out"].reshape(S, n_mels, out_ld), rows=rows, J=st["J"].copy())


def _is_canary(a):
    return (N.bits(a) == CAN).all()


def _check(got, streams, n_mels, p, normalize):
    """the operand bit for bit; raw, mean, std, out within the bound, every element; canaries everywhere else"""
    S, rows = len(streams), got["rows"]
    op = got["operand"]
    assert len(op) == S * rows * 160 + 512 and (op[S * rows * 160:] == 0).all()
    worst = 0.0
    for k, (row, ranges) in enumerate(streams):
        y = N.preemphasised(np.asarray(row, np.float32), ranges, p)
        want = np.zeros(rows * 160, np.float32)
        want[256:256 + len(y)] = y
        _same_bits(op[k * rows * 160:(k + 1) * rows * 160], want, f"operand of speaker {k}")
        J = len(y) // 160
        assert int(got["J"][k]) == J
        assert _is_canary(got["raw"][k, :, J:]) and _is_canary(got["out"][k, :, J:])
        if J == 0:
            assert _is_canary(got["mean"][k]) and _is_canary(got["std"][k])
            continue
        ref = N.reference(row, ranges, n_mels, p, normalize)
        assert ref.raw.shape == (n_mels, J)
        d_raw = np.abs(got["raw"][k, :, :J].astype(np.float64) - ref.raw)
        assert np.isfinite(got["raw"][k, :, :J]).all() and (d_raw <= ref.e_raw).all(), (k, float((d_raw / ref.e_raw).max()))
        if not normalize:
            N.bound(ref, True)    # (leaves e_mean and e_std: the statistics are written in both modes)
        assert (np.abs(got["mean"][k] - ref.mean) <= ref.e_mean).all(), k
        assert (np.abs(got["std"][k] - ref.std) <= ref.e_std).all(), k
        d = np.abs(got["out"][k, :, :J].astype(np.float64) - ref.out)
        assert np.isfinite(got["out"][k, :, :J]).all() and (d <= ref.bound).all(), (k, float((d / ref.bound).max()))
        worst = max(worst, float((d / ref.bound).max()))
        if not normalize:
            _same_bits(got["out"][k, :, :J], got["raw"][k, :, :J], "normalize == 0 hands out the raw rows")
    return worst


def _one_range(kind, n, seed=0):
    return N.signal(kind, n, seed), np.array([[0, n]], np.int64).reshape(-1, 2)[: 1 if n else 0]


@pytest.mark.parametrize("n", N.EDGE_LENGTHS)
def test_edge_lengths(handle, n):
    """0, 159, 160, 319, 320 samples: 0, 0, 1, 1, 2 frames; one frame has std 0 and the output exactly 0"""
    s = [_one_range("noise", n, 1)]
    got = _run(handle, s, 80, 0.97, True)
    assert int(got["J"][0]) == n // 160 == (0, 0, 1, 1, 2)[N.EDGE_LENGTHS.index(n)]
    _check(got, s, 80, 0.97, True)
    if n // 160 == 1:
        assert (got["std"][0] == 0).all() and (got["out"][0, :, 0] == 0).all()


@pytest.mark.parametrize("frames", N.TILE_FRAMES + N.REDUCE_FRAMES)
def test_tile_and_reduction_widths(handle, frames):
    """31, 32, 33 frames around the mel tile; 255, 256, 257 and 1025 around the widths of the statistics' strided partials"""
    n = frames * 160 + 77
    n_mels = 128 if frames in (32, 257) else 80
    s = [_one_range("speechlike" if frames > 100 else "noise", n, frames)]
    got = _run(handle, s, n_mels, 0.97, True)
    assert int(got["J"][0]) == frames
    print("frames", frames, "worst d / bound", _check(got, s, n_mels, 0.97, True))


@pytest.mark.parametrize("S,n_mels,p,normalize,wav_off", ((1, 80, 0.97, True, 0), (3, 128, 0.97, True, 1), (3, 80, 0.0, True, 2),
                                                          (1, 128, 0.0, False, 3), (3, 80, 0.97, False, 0)))
def test_seams_speakers_banks_and_alignment(handle, S, n_mels, p, normalize, wav_off):
    """run tables of 256-sample ranges: a frame spans three ranges, every seam lies inside the pre-emphasis; speakers of
    different lengths (one of them with gaps between its ranges, one empty with S == 3); rows at every alignment"""
    lens = (5000, 0, 7777)[:S] if S == 3 else (6000,)
    streams = []
    for k, n in enumerate(lens):
        row = N.signal(("noise", "tones", "speechlike")[k], n + 600, seed=k)
        assert n == 0 or row[0] != 0
        if k == 2:   # ranges of 256 with gaps of 64 between them: the seam's previous sample is NOT the row's previous sample
            ranges = np.array([[a, a + 256] for a in range(0, n, 320)], np.int64)
        else:
            ranges = N.blocks_of(n)
        streams.append((row, ranges))
    got = _run(handle, streams, n_mels, p, normalize, wav_off=wav_off)
    print("worst d / bound", _check(got, streams, n_mels, p, normalize))


def test_silence_and_a_constant_row(handle):
    """digital silence: every raw value is the one float32 the device's logf makes of 2^-24 (within its 2 ulp of ln 2^-24), std is
    0 and the output exactly 0.  A constant row: the frames that lie wholly inside it see one and the same operand, so their raw
    values are equal bit for bit; everything within the bound."""
    n = 3300
    s = [(np.zeros(n, np.float32), np.array([[0, n]], np.int64)), (N.signal("constant", n), np.array([[0, n]], np.int64))]
    got = _run(handle, s, 80, 0.97, True)
    _check(got, s, 80, 0.97, True)
    J = n // 160
    raw0 = got["raw"][0, :, :J]
    lnG = np.float32(np.log(2.0 ** -24))
    assert (N.bits(raw0) == N.bits(raw0[:1, :1])).all() and abs(float(raw0[0, 0]) - float(lnG)) <= 2 * abs(float(np.spacing(lnG)))
    assert (got["std"][0] == 0).all() and (got["mean"][0] == raw0[0, 0]).all() and (got["out"][0, :, :J] == 0).all()
    inner = got["raw"][1, :, 2:J - 3]                      # frames 2 .. : padded samples from 320 on, past the 256 zeros and y[0]
    assert (N.bits(inner) == N.bits(inner[:, :1])).all()


def test_one_launch_or_part_of_a_larger_one_same_bits(handle):
    """the same row alone (S = 1) and as the middle speaker of S = 3, behind another row offset: the same bits everywhere"""
    row, ranges = N.signal("speechlike", 9000, 7), N.blocks_of(8200)
    others = [_one_range("noise", 12000, 3), _one_range("tones", 4000, 4)]
    alone = _run(handle, [(row, ranges)], 80, 0.97, True, wav_off=0)
    among = _run(handle, [others[0], (row, ranges), others[1]], 80, 0.97, True, wav_off=3)
    J = int(alone["J"][0])
    assert J == 8200 // 160 == int(among["J"][1])
    for name in ("raw", "out"):
        _same_bits(alone[name][0, :, :J], among[name][1, :, :J], name)
    _same_bits(alone["mean"][0], among["mean"][1], "mean")
    _same_bits(alone["std"][0], among["std"][1], "std")
    # and with more operand rows than the path would give (another grid of every kernel)
    wide = _run(handle, [(row, ranges)], 80, 0.97, True, extra_rows=70)
    for name in ("raw", "out"):
        _same_bits(alone[name][0, :, :J], wide[name][0, :, :J], name + " (wider grid)")
    _same_bits(alone["std"][0], wide["std"][0], "std (wider grid)")


def test_refusals(handle):
    L = pkg("_lib")
    row, ranges = _one_range("noise", 2000)
    for edit in (dict(n_mels=64), dict(preemphasis=1.0), dict(preemphasis=-0.1), dict(preemphasis=float("nan")), dict(rows=3), dict(S=5),
                 dict(wav_off=4), dict(normalize=2)):
        regs, offs, A, n = N.run_table(ranges, 2)
        st = np.zeros(1, L.HANDOFF_STATE)
        st["A"], st["J"] = A, A // 160
        rows = A // 160 + 4
        job = dict(S=1, n_mels=80, normalize=1, cap_ranges=2, wav_off=0, preemphasis=0.97, wav_ld=len(row), rows=rows, raw_ld=rows - 4,
                   out_ld=rows - 4, wav=np.concatenate([row, np.zeros(8, np.float32)]), regs=regs, offs=offs, st=st, n_ranges=np.array([n], np.int32),
                   operand=N.canary(rows * 160 + 512), raw=N.canary(128 * rows), mean=N.canary(128), stdv=N.canary(128), out=N.canary(128 * rows))
        job.update(edit)
        with pytest.raises(L.CssError) as e:
            handle.nemo_kernels(job)
        assert e.value.code == L.CSS_ERR_INVALID_ARG, edit
        assert all(_is_canary(a) for a in e.value.left.values()), edit
