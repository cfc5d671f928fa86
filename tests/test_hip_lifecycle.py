"""The life cycle of a handle on the MI355X: whatever a handle and its streams allocate on the device goes back when the handle is
destroyed, whichever of its parts came to life and whatever was still open (csrc/api_ctx.hpp: every device buffer, page-locked
block and event is a member of an owner; css_destroy enumerates nothing).  Only the public Python API is used.

What the first test cannot see: a leak below a quarter of its margin per cycle (the margin is spread over four cycles), i.e. a
small table or an event -- and, with the margin the runtime's own drift forces (DRIFT_PARENT below), a buffer of up to about
40 MB.  tests/test_ownership_host.py covers that part on the sources: nothing outside the owners can release, or forget to
release, a resource."""
import gc

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

HANDOFF = dict(n_mels=80, pad_frames=8, drop_silence=True)
# f1 - f5 of this file on the build before the owners (hand-kept free lists, checked against the members: nothing leaked), one
# MI355X: 81 788 928 bytes over four cycles at a footprint F of 1 776 287 744.  That is more than F / 200, so the rule of
# DESIGN.md 1 applies: the margin is twice that drift instead of F / 100.  (With the owners: the same 81 788 928, cycle by cycle --
# not a buffer of either build; the likely holder is the runtime, per created and destroyed handle.)
DRIFT_PARENT = 81788928


def _rec(seconds, seed):
    return np.ascontiguousarray(pkg("synth").synth_meeting(float(seconds), 7, seed=seed)[0], dtype=np.float32)


def _free():
    import torch
    return int(torch.cuda.mem_get_info(0)[0])


@pytest.fixture(scope="module")
def audio():
    """three 6 s recordings, 5 s for the streams (float, PCM16, and 5 s worth of samples taken as 48 kHz input)"""
    x5 = _rec(5.0, 24)
    return {"run": [_rec(6.0, 21 + i) for i in range(3)], "f32": x5, "i16": np.round(np.clip(x5, -1.0, 1.0) * 32767.0).astype(np.int16),
            "f48": _rec(15.0, 25)}


def _cycle(state, audio, probe=None):
    """One handle with every kind of allocation alive -- a pass, a queued group of two (session slots, X_alt), both weight
    images, three streams (plain, hand-off, rate + hand-off; float, PCM16 and grouped pushes, a preview with hand-off) --
    destroyed with two streams open, one of them unfinished.  probe() is called where the device holds the most."""
    L, CSS, S = pkg("_lib"), pkg("css"), pkg("stream")
    sep = pkg("separator").HipSeparator(state[0], None, device=0)
    cfg = CSS.CssCfg()
    h = sep.handle
    rc = CSS.make_run_cfg(cfg, 16000, 7)
    h.run(audio["run"][0], rc)
    n_out = L.plan(sep.desc, rc, audio["run"][1].shape[0]).n_out
    pins = [(L.pinned_copy(x), L.pinned_empty((sep.desc.num_spks, n_out))) for x in audio["run"][1:]]
    for x, out in pins:
        h.run_enqueue(x, rc, out)
    h.wait()
    h.set_linear_mode("split_f16")
    h.set_linear_mode("exact_f32")
    plain, ho, rate = S.CssStream(sep, cfg), S.CssStream(sep, cfg, handoff=HANDOFF), S.CssStream(sep, cfg, handoff=HANDOFF, input_rate=48000)
    group = S.CssStreamGroup([plain, rate])
    for k in range(10):   # 5 s in chunks of 0.5 s
        group.push([audio["f32"][k * 8000:(k + 1) * 8000], audio["f48"][k * 24000:(k + 1) * 24000]])
        ho.push_pcm16(audio["i16"][k * 8000:(k + 1) * 8000])
    ho.preview(handoff=True)
    plain.finish()
    ho.finish()
    if probe:
        probe()
    plain.close()
    sep.close()   # `ho` (finished) and `rate` (unfinished) are still open
    del pins
    gc.collect()


def test_destroy_returns_the_device_memory(mc_state, audio):
    """Five cycles.  Free device memory f0 before the first, f_peak at its fullest point (footprint F = f0 - f_peak), f1 after
    it, f5 after the fifth: f5 >= f1 - margin, margin = 2 * DRIFT_PARENT (it would be F / 100 if create / destroy cycles did
    not drift by more than F / 200 on their own).  The first cycle is not part of the comparison: it also loads the code
    objects and fills the runtime's own pools.  A set of buffers that leaks once per cycle shows as four times its size."""
    _free()
    f0 = _free()
    peak = []
    _cycle(mc_state, audio, probe=lambda: peak.append(_free()))
    after = [_free()]
    for _ in range(4):
        _cycle(mc_state, audio)
        after.append(_free())
    f1, f5 = after[0], after[-1]
    F = f0 - peak[0]
    margin = 2 * DRIFT_PARENT
    print(f"lifecycle: f0 {f0} f_peak {peak[0]} after cycles 1..5 {after}  F {F} ({F / 2**20:.1f} MiB)  f1 - f5 {f1 - f5}  "
          f"F/100 {F // 100}  margin {margin}")
    assert F > 0
    assert f5 >= f1 - margin, (f1 - f5, margin, F)


def test_new_handle_after_destroy_starts_clean(mc_state):
    """A handle destroyed with a stream open leaves nothing behind for the next one: its first stream gets id 0 and returns
    css_run's output of a 4 s recording, bit for bit."""
    CSS, S = pkg("css"), pkg("stream")
    cfg = CSS.CssCfg()
    x = _rec(4.0, 31)
    old = pkg("separator").HipSeparator(mc_state[0], None, device=0)
    left_open = S.CssStream(old, cfg)
    left_open.push(x[:20000])
    old.close()
    sep = pkg("separator").HipSeparator(mc_state[0], None, device=0)
    ref = sep.handle.run(x, CSS.make_run_cfg(cfg, 16000, 7)).copy()
    s = S.CssStream(sep, cfg)
    assert s.id == 0
    got = np.concatenate([np.stack(s.push(x)), np.stack(s.finish())], axis=1)
    assert got.shape == ref.shape and np.array_equal(got, ref)
    sep.close()
