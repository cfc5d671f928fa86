"""tests/nemo_reference.py on the CPU: the float64 definition against a torch.stft float32 rendering of the published class body
(transformers' ParakeetFeatureExtractor; the class itself needs librosa to load, so its arithmetic is restated here), the bank
against transformers.audio_utils.mel_filter_bank, the float32 restatement of the device path and the package's numpy statement
inside the counted bound, and every named mistake outside it on at least one listed case."""
import numpy as np
import pytest

import nemo_reference as N
from conftest import pkg

CASES = (   # (name, signal, samples, ranges or None = one range, n_mels, preemph)
    ("noise_one_range", "noise", 16000, None, 80, 0.97),
    ("speech_blocks", "speechlike", 12000, "blocks", 80, 0.97),
    ("tones_two_ranges", "tones", 9000, ((100, 3000), (4000, 9000)), 128, 0.97),
    ("noise_no_preemph", "noise", 4000, "blocks", 128, 0.0),
    ("quiet_around_the_guard", "quiet", 8000, None, 80, 0.97),
)


def _case(c):
    name, kind, n, ranges, n_mels, p = c
    row = N.signal(kind, n, seed=len(name))
    if ranges is None:
        ranges = [[0, n]]
    elif ranges == "blocks":
        ranges = N.blocks_of(n)
    return row, np.asarray(ranges, np.int64), n_mels, p


def _torch_rendering(x, bank, preemph, normalize):
    """the body of ParakeetFeatureExtractor.__call__ / _torch_extract_fbank_features for one utterance, float32"""
    torch = pytest.importorskip("torch")
    w = torch.from_numpy(np.ascontiguousarray(x, np.float32))[None, :]
    if preemph:
        w = torch.cat([w[:, :1], w[:, 1:] - preemph * w[:, :-1]], dim=1)
    window = torch.hann_window(400, periodic=False)
    stft = torch.stft(w, 512, hop_length=160, win_length=400, window=window, return_complex=True, pad_mode="constant")
    mag = torch.sqrt(torch.view_as_real(stft).pow(2).sum(-1)).pow(2)
    mel = torch.log(torch.from_numpy(bank.astype(np.float32)) @ mag + 2 ** -24).permute(0, 2, 1)      # [1][frames][n_mels]
    L = (x.shape[0] + 512 // 2 * 2 - 512) // 160
    if not normalize:
        return mel[0, :L].T.numpy()
    mask = (torch.arange(mel.shape[1])[None, :] < L).unsqueeze(-1)
    masked = mel * mask
    mean = (masked.sum(dim=1) / L).unsqueeze(1)
    var = ((masked - mean) ** 2 * mask).sum(dim=1) / (L - 1)
    out = (mel - mean) / (torch.sqrt(var).unsqueeze(1) + 1e-5)
    return (out * mask)[0, :L].T.numpy()


@pytest.mark.parametrize("n_mels", (80, 128))
def test_definition_against_the_torch_rendering_of_the_published_class(n_mels):
    """The oracle tolerance is the counted bound itself, for the rendering's own path: an FFT rounds a term fewer times than
    the direct sum (513, and one more for torch's float32 window formula), the class takes a square root and squares it again
    (4 roundings per power), torch's logarithm is within the same 2 ulp, and its float32 statistics round at most once per
    term of their sums (k_stat = 1 per term: the sequential worst case)."""
    x = N.signal("speechlike", 64000, seed=3) + N.signal("noise", 64000, seed=4) * np.float32(1e-3)
    ref = N.reference(x, [[0, len(x)]], n_mels, 0.97, normalize=False)
    W = N.tables(n_mels)[1]
    got = _torch_rendering(x, W, 0.97, False)
    assert got.shape == ref.raw.shape == (n_mels, 400)
    b = N.bound(ref, False, k_prod=N.NFFT + 2, k_pow=4)
    d = np.abs(got - ref.raw)
    print("raw: max |d| %.3g, max d / bound %.3g, values %.2f .. %.2f" % (d.max(), (d / b).max(), ref.raw.min(), ref.raw.max()))
    assert (d <= b).all()
    refn = N.reference(x, [[0, len(x)]], n_mels, 0.97, normalize=True)
    gotn = _torch_rendering(x, W, 0.97, True)
    bn = N.bound(refn, True, k_prod=N.NFFT + 2, k_pow=4, k_stat=1.0)
    dn = np.abs(gotn - refn.out)
    print("normalised: max |d| %.3g, max d / bound %.3g" % (dn.max(), (dn / bn).max()))
    assert (dn <= bn).all()


@pytest.mark.parametrize("n_mels", (80, 128))
def test_bank_is_the_published_one(n_mels):
    au = pytest.importorskip("transformers.audio_utils")
    theirs = au.mel_filter_bank(257, n_mels, 0.0, 8000.0, 16000, norm="slaney", mel_scale="slaney").T.astype(np.float32)
    assert np.array_equal(N.mel_bank(n_mels).astype(np.float32), theirs)
    assert np.array_equal(pkg("stream").nemo_tables(n_mels)[1], theirs)


def test_package_tables_are_the_reference_tables():
    S = pkg("stream")
    for n_mels in (80, 128):
        A, W = N.tables(n_mels)
        a, w = S.nemo_tables(n_mels)
        assert a.dtype == w.dtype == np.float32 and np.array_equal(a, A.astype(np.float32)) and np.array_equal(w, W.astype(np.float32))
    w = N.window()
    assert (w[:56] == 0).all() and (w[456:] == 0).all() and w[56] == 0 and w[455] == 0 and np.array_equal(w[56:456], w[56:456][::-1])


@pytest.mark.parametrize("c", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("normalize", (True, False))
def test_float32_statements_lie_inside_the_bound(c, normalize):
    row, ranges, n_mels, p = _case(c)
    ref = N.reference(row, ranges, n_mels, p, normalize)
    raw, mean, std, out = N.model32(row, ranges, n_mels, p, normalize)
    assert out.shape == ref.out.shape and ref.out.shape[1] == sum(b - a for a, b in ranges) // 160
    assert (np.abs(out - ref.out) <= ref.bound).all()
    if normalize:
        assert (np.abs(mean - ref.mean) <= ref.e_mean).all() and (np.abs(std - ref.std) <= ref.e_std).all()
    pk = pkg("stream").nemo_features(N.concat(row, ranges), n_mels, p, normalize)
    assert pk.dtype == np.float32 and (np.abs(pk - ref.out) <= ref.bound).all()


def test_short_inputs():
    S = pkg("stream")
    for n in N.EDGE_LENGTHS:
        x = N.signal("noise", n)
        ref = N.reference(x, [[0, n]] if n else [], 80)
        assert ref.out.shape == (80, n // 160) == S.nemo_features(x, 80).shape
        if n // 160 == 1:   # one frame: std is taken as 0, the output is (v - v) / 1e-5 = 0
            assert (ref.std == 0).all() and (ref.out == 0).all() and (S.nemo_features(x, 80) == 0).all()
    z = N.reference(N.signal("zeros", 1600), [[0, 1600]], 80)
    # (the float64 mean of ten equal values is that value up to the sum's own rounding, 2^-53 relative)
    assert (z.raw == np.log(2.0 ** -24)).all() and np.abs(z.out).max() < 1e-8 and z.std.max() < 1e-13


def test_every_named_mistake_leaves_the_bound():
    """each switch of the reference, on the listed cases: at least one case where it lies outside the definition's bound"""
    refs = [(c, _case(c)) for c in CASES]
    for mut in N.MISTAKES:
        worst = 0.0
        for c, (row, ranges, n_mels, p) in refs:
            for normalize in (True, False):
                ref = N.reference(row, ranges, n_mels, p, normalize)
                m = N.reference(row, ranges, n_mels, p, normalize, mut=mut, want_bound=False)
                worst = max(worst, N.deviation(m, ref)[0])
        print(mut, worst)
        assert worst > 1.0, mut
