"""The values of the Whisper log-mel hand-off (css_handoff_logmel: csrc/handoff.hip's gather, the 402 x 416 product, the mel
tile and the normalisation) against the float64 reference and the derived bound of tests/handoff_reference.py (DESIGN.md 7 N4,
"The hand-off's values").  One finished pass of 6 s gives the handle its plan; after that every test writes a hand-made gate
(Handle.write(BUF_ACT_FINAL)), uploads three made-up waveforms [3][wav_ld] and calls the entry per stream.  Per call:

  shape      the frame count and the kept ranges the gate implies; the range rows behind n_regions keep their sentinel
  value      |got - reference| <= bound elementwise; the worst ratio of each call is printed
  bits       where the reference lies at the floor and the clamp below it: the float32 -1.5; elements that are surely clamped all
             hold one float32
  ownership  mel_host behind n_mels * frames floats keeps the canary 0x7FC0BEEF

tests/test_handoff_reference.py shows, on the CPU and on this module's own list of cases, that each of the twelve named mistakes
lies above the bound on at least one of them.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

import handoff_reference as H
from conftest import pkg

pytestmark = pytest.mark.gpu

TL, N_OUT = 374, 96000
SLACK = 256
SENT = -7
CASES = {c["name"]: c for c in H.cases(TL)}


@pytest.fixture(scope="module")
def world():
    """the 1-block model of tests/test_hip_frontend_kernels.py, one finished pass of 6 s on its handle"""
    import torch
    L, w, css = pkg("_lib"), pkg("weights"), pkg("css")
    if L.load().css_device_count() < 1:
        pytest.fail("no HIP device visible")
    desc = w.ModelDesc(num_blocks=1)
    sep = pkg("separator").HipSeparator(w.apply_golden_recipe(w.portable_state_dict(desc, 5)), None, device=0)
    h = sep.handle
    x = pkg("synth").synth_meeting(6.0, 7, seed=11)
    x = np.ascontiguousarray((x[0] if x.ndim == 3 else x)[:N_OUT], dtype=np.float32)
    rc = css.make_run_cfg(css.CssCfg(activity_th=0.3, show_progressbar=False), 16000, 7)
    n_out = int(L.plan(sep.desc, rc, x.shape[0]).n_out)
    pcm = torch.from_numpy(x).cuda()
    wav = torch.empty((3, n_out), dtype=torch.float32, device="cuda")
    h.run_device(pcm.data_ptr(), x.shape[0], 7, rc, wav.data_ptr(), n_out)
    torch.cuda.synchronize()
    assert int(h.get_plan().mix_frames) == TL and n_out == N_OUT == (TL + 1) * H.BLOCK
    worst = {}
    yield dict(h=h, L=L, torch=torch, worst=worst)
    for (kind, n_mels), r in sorted(worst.items()):
        print(f"hand-off values, worst error / bound: {kind} n_mels {n_mels}: {r:.4f}")
    sep.close()


def _upload(world, rows, ld_extra):
    """three waveforms as a device buffer [3][N_OUT + ld_extra] (ld_extra 1: rows 1 and 2 start off 16-byte boundaries)"""
    buf = np.zeros((3, N_OUT + ld_extra), np.float32)
    for k, r in enumerate(rows):
        buf[k, :N_OUT] = r
    return world["torch"].from_numpy(buf).cuda(), N_OUT + ld_extra


def _call(world, dev, wav_ld, stream, n_mels, pad, drop, frames, max_regions=8):
    """one css_handoff_logmel with mel_host of exactly n_mels * frames floats plus slack -> (mel [n_mels][frames], ranges)"""
    h, L = world["h"], world["L"]
    flat = H.canary(n_mels * frames + SLACK)
    regions = np.full((max_regions + 2, 2), SENT, np.int64)
    nfr, nreg = C.c_int64(-1), C.c_int32(-1)
    L.check(h.h, h.lib.css_handoff_logmel(h.h, C.c_void_p(dev.data_ptr()), wav_ld, stream, n_mels, pad, int(drop),
                                          flat.ctypes.data_as(C.c_void_p), frames, C.byref(nfr), regions.ctypes.data_as(C.c_void_p),
                                          max_regions, C.byref(nreg)))
    assert nfr.value == frames, ("frames", nfr.value, frames)
    assert (H.bits(flat[n_mels * frames:]) == H.CANARY).all(), "mel_host was written behind n_mels * frames floats"
    assert (regions[nreg.value:] == SENT).all(), "the range table was written behind n_regions rows"
    return flat[:n_mels * frames].reshape(n_mels, frames).copy(), regions[:nreg.value].copy()


def _judge(world, got, ref, kind, n_mels, what):
    """got against the reference: the bound, the exact elements, the clamped ones; returns and records the worst ratio"""
    assert got.shape == ref.out.shape and got.dtype == np.float32, (what, got.shape, ref.out.shape)
    assert np.isfinite(got).all(), (what, "a non-finite feature")
    err = np.abs(got.astype(np.float64) - ref.out)
    q = np.where(err == 0, 0.0, err / np.maximum(ref.bound, 1e-300))
    pos = np.unravel_index(int(q.argmax()), q.shape)
    print(f"{what}: worst error / bound {q[pos]:.4f} at band {pos[0]} frame {pos[1]} (error {err[pos]:.3g}, bound {ref.bound[pos]:.3g})")
    assert q[pos] <= 1.0, (what, f"ratio {q[pos]:.3f} at {pos}: got {got[pos]!r}, reference {ref.out[pos]!r}, bound {ref.bound[pos]!r}")
    stray = np.argwhere(ref.exact & (H.bits(got) != H.bits(np.float32(-1.5))))
    assert stray.size == 0, (what, f"{len(stray)} elements at the floor are not -1.5 bit for bit, the first at {stray[0]}: {got[tuple(stray[0])]!r}")
    cl = H.bits(got[ref.clamped])
    assert cl.size == 0 or (cl == cl[0]).all(), (what, "elements that are surely clamped hold different floats")
    key = (kind, n_mels)
    world["worst"][key] = max(world["worst"].get(key, 0.0), float(q[pos]))
    return float(q[pos])


@pytest.mark.parametrize("name", list(CASES))
def test_values(world, name):
    h, L, c = world["h"], world["L"], CASES[name]
    rows = [H.case_reference(c, row, TL, N_OUT) for row in range(3)]
    gates = np.stack([r[0] for r in rows])
    h.write(L.BUF_ACT_FINAL, gates)
    assert np.array_equal(h.read(L.BUF_ACT_FINAL), gates)
    dev, wav_ld = _upload(world, [r[2] for r in rows], c["ld_extra"])
    for row, (_, ranges, _, x, ref) in enumerate(rows):
        what = f"{name} stream {row} ({c['kinds'][row]}, n_mels {c['n_mels']}, wav_ld {wav_ld})"
        assert ref.nfr == len(x) // 160 > 0
        got, reg = _call(world, dev, wav_ld, row, c["n_mels"], c["pad"], c["drop"], ref.nfr)
        assert np.array_equal(reg, ranges), (what, reg, ranges)
        _judge(world, got, ref, c["kinds"][row], c["n_mels"], what)
        if c["kinds"][row] == "zeros":
            assert ref.exact.all() and (H.bits(got) == H.bits(np.float32(-1.5))).all(), (what, "silence is not -1.5 everywhere")


def test_filterbank_is_rebuilt_when_n_mels_changes(world):
    """80 -> 128 -> 80 -> 128 -> 128 -> 80 on one handle: the cached filterbank follows, the values are right each time and a
    repeated call returns the same bits"""
    h, L = world["h"], world["L"]
    c = CASES["21_blocks_2_runs"]
    rows = [H.case_reference(c, row, TL, N_OUT) for row in range(3)]
    assert c["kinds"][2] == "noise"
    h.write(L.BUF_ACT_FINAL, np.stack([r[0] for r in rows]))
    dev, wav_ld = _upload(world, [r[2] for r in rows], 1)
    x = rows[2][3]
    refs = {n_mels: H.reference(x, n_mels) for n_mels in (80, 128)}
    seen = {}
    for i, n_mels in enumerate((80, 128, 80, 128, 128, 80)):
        got, _ = _call(world, dev, wav_ld, 2, n_mels, c["pad"], c["drop"], refs[n_mels].nfr)
        _judge(world, got, refs[n_mels], "noise", n_mels, f"call {i} with n_mels {n_mels}")
        if n_mels in seen:
            assert np.array_equal(H.bits(got), H.bits(seen[n_mels])), (i, n_mels, "a repeated call returned other bits")
        seen[n_mels] = got


@pytest.mark.parametrize("offset", (0, 85))
def test_nan_sample_reads_as_floor_frames(world, offset):
    """What the device path does with a NaN sample today (INTEGRATION.md states it; Whisper itself would propagate the NaN): the
    frames whose operand row holds it read as floor frames -- fmaxf(NaN, 1e-10f) is 1e-10f, so every band is
    (max(-10, maximum - 8) + 4) / 4 -- and no other frame changes a bit.  An operand row is the frame's 400 samples and the 16
    that pad the product's K to 416 (zero matrix columns, and 0 * NaN is NaN): at offset 85 the sample lies in two frames'
    samples and in the padding of a third."""
    h, L = world["h"], world["L"]
    c = CASES["whole_128"]
    rows = [H.case_reference(c, row, TL, N_OUT) for row in range(3)]
    assert c["kinds"][0] == "noise" and not c["drop"]
    ref = rows[0][4]
    h.write(L.BUF_ACT_FINAL, np.stack([r[0] for r in rows]))
    dev, wav_ld = _upload(world, [r[2] for r in rows], 0)
    base, _ = _call(world, dev, wav_ld, 0, 128, c["pad"], False, ref.nfr)
    q = 160 * 300 + offset                                   # the sample's place in the padded concatenation
    bad = rows[0][2].copy()
    bad[q - 200] = np.nan
    dev2, _ = _upload(world, [bad, rows[1][2], rows[2][2]], 0)
    got, _ = _call(world, dev2, wav_ld, 0, 128, c["pad"], False, ref.nfr)
    j = np.arange(ref.nfr)
    holds = (160 * j <= q) & (q < 160 * j + 416)
    in_window = (160 * j <= q) & (q < 160 * j + 400)
    assert holds.sum() == 3 and in_window.sum() == (3 if offset == 0 else 2) and not (in_window & ~holds).any()
    assert not holds[int(np.unravel_index(int(ref.raw.argmax()), ref.raw.shape)[1])]       # the maximum is another frame's
    assert np.isfinite(got).all()
    assert np.array_equal(H.bits(got[:, ~holds]), H.bits(base[:, ~holds])), "a frame without the NaN sample changed bits"
    fl = got[:, holds]
    assert (H.bits(fl) == H.bits(fl[0, 0])).all(), "the frames that hold the NaN sample are not one value"
    want = (max(-10.0, ref.mx - 8.0) + 4.0) / 4.0
    tol = H.SECOND * ((ref.e_mx + H.U * abs(ref.mx - 8.0)) / 4 + 2 * H.U * abs(want))
    assert abs(float(fl[0, 0]) - want) <= tol, (float(fl[0, 0]), want, tol)
