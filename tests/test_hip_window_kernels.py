"""Every launch form of the window kernels and the queued sessions' hand-off kernels of csrc/handoff.hip through the host entries of
include/css_mi355_handoff_kernels.h, against the exact models of tests/window_reference.py (DESIGN.md 7b "The window and session
hand-off kernels, launch form by launch form").  Every comparison is bit for bit; there is no tolerance in this file.  Three kinds
of assertion per launch:

  ownership  every output allocation and 256 elements of slack behind it (and the elements of its offset in front) start as the
             canary of its type (0x7FC0BEEF, 0x5A5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A); the WHOLE allocation is compared with the
             model's, so everything the launch does not own keeps its bits.  Inputs the model does not read can show a wrong
             read: frames outside a span, mel columns at or past min(J, max_frames), provisional columns at or past P and maximum
             slots outside the span are +inf (not NaN: fmaxf turns a NaN frame into the clamp's floor and a NaN maximum into
             nothing); wav samples around the rows are NaN; one case apiece puts a NaN frame INSIDE a span and expects the floor
  value      bit equality with the model
  bits       a speaker (an item) in a table against the same alone

Coverage, one line per launcher and template instance:
  launch_session_keep_scan                 test_scan: TL 1 .. 5, 1019 .. 1029, 2047 .. 2050, 3073 x gate_off 0 .. 3 x S 1 .. 4 x pad 0, 1, 3, 300,
                                           4096 x ten kinds of gate (none, all, first, last, gaps of 2 pad + 1 and 2 pad + 2, runs ending and
                                           starting at frames 1023 / 1024 / 1025 under every row alignment, bytes 0x80 and 0xFF, random);
                                           cap_ranges at the path's bound, the run count, the count - 1 and 1; drop off; a row alone
  launch_session_gather                    test_gather: the scan cases' own tables (the over-capacity ones too), rows as on the path and
                                           one more, wav_off 0 .. 3; A of 1, 201, 256, 512; A = 0; no run; equal offs; a speaker alone
  launch_session_norm                      test_norm: maxima positive, negative, zero; J 0, 1, 255, 256, 257, rows; out_ld below and above
                                           J; rows = 0 (no launch)
  launch_session_windows                   test_session_windows: (96, 64), (64, 7), (5, 5), (9, 1), (3000, 3000); ld width .. width + 3; J 0, 1, 3,
                                           stride - 1, stride, stride + 1, above max_frames; whole absent, J, 4095, 4096, 4097, 8197 with J
                                           4090 .. 4100; win absent; n_mels 5, 8, 9, 80, 128
    session_window_row<float>  (V = 4)     ... every mel_off 0 .. 3 x win_off 0 .. 7 (whole_off too), float32
    session_window_row<__half> (V = 8)     ... the same, float16; ties to even in both directions (test_ties)
  launch_stream_windows                    test_stream_windows: hist 1, 3, 4, 7, 8, 9, 32, 33, 50 x J 0, 1, hist - 1, hist, hist + 1, 2 hist + 3,
                                           2^32 + 5 x no provisional frames, P 0, 1, 5, pv_ld, *n_new above pv_ld; spans in the ring, across
                                           the wrap and across the seam at every position of a group, wholly provisional; widths 1 .. 17 and
                                           3000; tables of 33 (two launches) and 64 items with repeats and n_mels 5, 8, 9, 80, 128 mixed
    window_row<float>  (V = 4)             ... every ring_off, pv_off 0 .. 3 x out_off 0 .. 7, float32
    window_row<__half> (V = 8)             ... the same, float16; ties; a NaN frame in the ring and in the provisional frames
  the entries' refusals                    test_refusals
Needs an MI355X."""
import numpy as np
import pytest

import window_reference as W
from conftest import pkg

pytestmark = pytest.mark.gpu


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
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    assert a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.size == 0:
        return
    ua, ub = a.view(np.uint8).reshape(a.size, -1), b.view(np.uint8).reshape(b.size, -1)
    diff = np.flatnonzero((ua != ub).any(axis=-1))
    assert diff.size == 0, (what, f"{len(diff)} of {a.size} values differ, the first at {diff[0]}: {a[diff[0]]!r} != {b[diff[0]]!r}")


def _same_all(got, want, what):
    for k, v in want.items():
        _same_bits(got[k], v, (what, k))


# ---- the keep-scan ------------------------------------------------------------------------------------------------------------------

SCAN_FIELDS = ("S", "TL", "pad", "drop", "cap_ranges", "gate_off")


def _scan_job(c, blank):
    return dict({k: c[k] for k in SCAN_FIELDS}, gate=c["gate"], **blank)


def test_scan(handle):
    cases = W.scan_cases()
    for c in cases:
        blank = W.scan_blank(c)
        _same_all(handle.session_scan(_scan_job(c, blank)), W.scan(c, blank), c["name"])
    # a row of a table against the row alone, at the alignment it has in the table
    for c in [c for c in cases if c["S"] > 1][::9]:
        S, TL, cap = c["S"], c["TL"], c["cap_ranges"]
        table = handle.session_scan(_scan_job(c, W.scan_blank(c)))
        for k in range(S):
            a = (c["gate_off"] + k * TL) & 3
            row = c["gate"][c["gate_off"] + k * TL:c["gate_off"] + (k + 1) * TL]
            one = dict(c, S=1, gate_off=a, gate=np.concatenate([np.full(a, W.CANARY_BYTE, np.uint8), row, np.full(W.SLACK, W.CANARY_BYTE, np.uint8)]))
            alone = handle.session_scan(_scan_job(one, W.scan_blank(one)))
            for name, n in (("psum", TL + 1), ("regs", 2 * cap), ("offs", cap), ("st", 1), ("n_new", 1), ("n_ranges", 1), ("ranges_out", 2 * cap),
                            ("n_frames_out", 1), ("n_ranges_out", 1)):
                _same_bits(table[name][k * n:(k + 1) * n], alone[name][:n], (c["name"], k, name, "alone"))


# ---- the gather ---------------------------------------------------------------------------------------------------------------------

GATHER_FIELDS = ("S", "cap_ranges", "wav_off", "wav_ld", "rows", "regs", "offs", "st", "n_ranges", "wav")


def _gather_job(c):
    return dict({k: c[k] for k in GATHER_FIELDS}, operand=W.canary(c["S"] * c["rows"] * 160 + 416))


def test_gather(handle):
    cases = W.gather_cases()
    for c in cases:
        job = _gather_job(c)
        got = handle.session_gather(job)["operand"]
        _same_bits(got, W.gather(c, job["operand"]), c["name"])
    for c in [c for c in cases if c["S"] > 1][::5]:
        S, cap, per = c["S"], c["cap_ranges"], c["rows"] * 160
        table = handle.session_gather(_gather_job(c))["operand"]
        for k in range(S):
            one = dict(c, S=1, regs=c["regs"][k * cap * 2:(k + 1) * cap * 2], offs=c["offs"][k * cap:(k + 1) * cap], st=c["st"][k:k + 1],
                       n_ranges=c["n_ranges"][k:k + 1],
                       wav=np.concatenate([c["wav"][:c["wav_off"]], c["wav"][c["wav_off"] + k * c["wav_ld"]:c["wav_off"] + (k + 1) * c["wav_ld"]]]))
            alone = handle.session_gather(_gather_job(one))["operand"]
            _same_bits(table[k * per:(k + 1) * per], alone[:per], (c["name"], k, "alone"))


# ---- the normalisation --------------------------------------------------------------------------------------------------------------

def test_norm(handle):
    for c in W.norm_cases():
        out = W.canary(c["S"] * c["n_mels"] * c["out_ld"] + W.SLACK)
        job = dict({k: c[k] for k in ("S", "n_mels", "mel_ld", "out_ld", "rows", "st", "mel")}, out=out)
        _same_bits(handle.session_norm(job)["out"], W.session_norm(c, out), c["name"])


# ---- session windows ----------------------------------------------------------------------------------------------------------------

SW_FIELDS = ("S", "n_mels", "width", "stride", "f16", "win_off", "whole_off", "mel_off", "mel_ld", "max_frames", "ld", "cap_windows", "whole_ld")


def _sw_job(c, blank):
    return dict({k: c[k] for k in SW_FIELDS}, st=c["st"], mel=c["mel"], **blank)


def _sw_run(handle, c):
    blank = W.session_windows_blank(c)
    got = handle.session_windows(_sw_job(c, blank))
    assert got["n_win_jobs"] == (-(-c["max_frames"] // c["stride"]) if "win" in blank else 0), c["name"]
    assert got["n_whole_jobs"] == (-(-c["whole_ld"] // W.WHOLE_CHUNK) if "whole" in blank else 0), c["name"]
    return got, blank


def test_session_windows(handle):
    cases = W.session_window_cases()
    for c in cases:
        got, blank = _sw_run(handle, c)
        _same_all(got, W.session_windows(c, blank), c["name"])
    for c in [c for c in cases if "align" in c["name"]][::7]:          # a speaker of the table against the speaker alone
        S, nm = c["S"], c["n_mels"]
        table, _ = _sw_run(handle, c)
        for k in range(S):
            lead = (c["mel_off"] + k * nm * c["mel_ld"]) & 3              # (the speaker's rows keep their alignment)
            rows = c["mel"][c["mel_off"] + k * nm * c["mel_ld"]:c["mel_off"] + (k + 1) * nm * c["mel_ld"]]
            n_win, n_whole = c["cap_windows"] * nm * c["ld"], nm * c["whole_ld"]
            w_at, h_at = c["win_off"] + k * n_win, c["whole_off"] + k * n_whole
            one = dict(c, S=1, st=c["st"][k:k + 1], mel_off=lead, mel=np.concatenate([np.full(lead, np.inf, np.float32), rows, np.full(8, np.inf, np.float32)]),
                       win_off=w_at % 8, whole_off=h_at % 8)
            alone, _ = _sw_run(handle, one)
            _same_bits(table["win"][w_at:w_at + n_win], alone["win"][one["win_off"]:one["win_off"] + n_win], (c["name"], k, "win alone"))
            _same_bits(table["whole"][h_at:h_at + n_whole], alone["whole"][one["whole_off"]:one["whole_off"] + n_whole], (c["name"], k, "whole alone"))
            assert table["n_windows_out"][k] == alone["n_windows_out"][0]


# ---- stream windows -----------------------------------------------------------------------------------------------------------------

ITEM_FIELDS = ("n_frames", "width", "n_mels", "f16", "ring_off", "pv_off", "out_off", "hist", "ld", "J", "pv_ld", "ring", "fmax")


def _item_job(it, out):
    job = dict({k: it[k] for k in ITEM_FIELDS}, out=out)
    if it.get("pv") is not None:
        job.update(pv=it["pv"], pvmax=it["pvmax"], n_new=it["n_new"])
    return job


def _run_table(handle, items, what):
    blanks = [W.stream_out_blank(it) for it in items]
    res0 = W.canary_res(len(items) + 8)
    left, res = handle.stream_windows([_item_job(it, b) for it, b in zip(items, blanks)], res0)
    want_res = res0.copy()
    for i, (it, b) in enumerate(zip(items, blanks)):
        out, want_res[i] = W.stream_window(it, b, res0[i])
        _same_bits(left[i]["out"], out, (what, i, it["name"], "out"))
    _same_bits(res.view(np.int32), want_res.view(np.int32), (what, "res"))
    return left, res


def test_stream_windows(handle):
    alone = {}
    for name, items in W.stream_tables():
        assert len(items) <= 64
        left, res = _run_table(handle, items, name)
        if name.startswith("table_"):                    # an item of a table (a repeat among them) against the item alone
            for i, it in enumerate(items):
                if id(it) not in alone:
                    l1, r1 = _run_table(handle, [it], it["name"])
                    alone[id(it)] = (l1[0]["out"], r1[0])
                _same_bits(left[i]["out"], alone[id(it)][0], (name, i, "alone"))
                assert res[i].tobytes() == alone[id(it)][1].tobytes(), (name, i, "alone")


def test_ties(handle):
    """raw 2^-9 under a maximum of 8 is 1 + 2^-11 in float32, a tie that float16 rounds to 1.0; 3 x 2^-9 is 1 + 3 x 2^-11, a tie that
    rounds up to 1 + 2^-9; a NaN frame inside a span takes the floor"""
    half = lambda a: np.ascontiguousarray(a).view(np.float16).astype(np.float64).tolist()
    for c in W.tie_cases_session():
        if "ties" not in c["name"]:
            continue
        got, _ = _sw_run(handle, c)
        row = got["win"][c["win_off"]:c["win_off"] + 4]
        assert (half(row) if c["f16"] else row.astype(np.float64).tolist()) == \
            ([1.0, 1 + 2.0 ** -9, 3.0, 1.0] if c["f16"] else [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 3.0, 1.0]), c["name"]
    for it in W.tie_items():
        left, res = _run_table(handle, [it], it["name"])
        out = left[0]["out"]
        if "ties" in it["name"]:
            row = out[it["out_off"]:it["out_off"] + 4]
            assert (half(row) if it["f16"] else row.astype(np.float64).tolist()) == \
                ([1.0, 1 + 2.0 ** -9, 1 + 2.0 ** -9, 1.0] if it["f16"] else [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 5 * 2.0 ** -11, 1.0]), it["name"]
            assert res[0]["window_max"] == 8.0
        else:
            body = out[it["out_off"]:it["out_off"] + it["n_mels"] * it["ld"]].reshape(it["n_mels"], it["ld"])[:, :it["width"]]
            vals = body.view(np.float16).astype(np.float32) if it["f16"] else body
            assert not np.isnan(vals).any() and (vals == (res[0]["window_max"] - np.float32(8) + np.float32(4)) * np.float32(0.25)).any(), it["name"]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def _refused(call, job, what):
    L = pkg("_lib")
    jobs = job if isinstance(job, list) else [job]
    before = [{k: v.copy() for k, v in j.items() if isinstance(v, np.ndarray)} for j in jobs]
    with pytest.raises(L.CssError) as e:
        call(job)
    assert e.value.code == L.CSS_ERR_INVALID_ARG and "_host: " in str(e.value), (what, str(e.value))
    left = e.value.left[0] if isinstance(e.value.left, tuple) else e.value.left
    left = left if isinstance(left, list) else [left]
    for j, b, l in zip(jobs, before, left):
        for k, v in b.items():
            _same_bits(j[k].view(np.uint8), v.view(np.uint8), what + ": the caller's " + k)
            if k in l:
                _same_bits(l[k].view(np.uint8), v.reshape(-1).view(np.uint8), what + ": " + k + " as the call left it")


def test_refusals(handle):
    # ---- scan
    c = [c for c in W.scan_cases() if c["name"].startswith("scan_cap_minus_1_TL1029_dense_S3")][0]
    scan = lambda **kw: dict(_scan_job(c, W.scan_blank(c)), **kw)
    handle.session_scan(scan())                      # (accepted: a capacity below the run count)
    for kw in (dict(TL=0), dict(pad=-1), dict(pad=4097), dict(cap_ranges=0), dict(gate_off=4), dict(gate_off=-1), dict(S=0), dict(S=5),
               dict(gate=c["gate"][:c["gate_off"] + c["S"] * c["TL"] - 1]), dict(psum=W.scan_blank(c)["psum"][:c["S"] * (c["TL"] + 1) - 1]),
               dict(regs=W.scan_blank(c)["regs"][:c["S"] * c["cap_ranges"] * 2 - 1]), dict(st=W.canary_state(c["S"] - 1)),
               dict(ranges_out=W.scan_blank(c)["ranges_out"][:1])):
        _refused(handle.session_scan, scan(**kw), f"scan: {sorted(kw)}")
    # ---- gather
    g = [g for g in W.gather_cases() if g["name"] == "gather_equal_offs"][0]
    gather = lambda **kw: dict(_gather_job(g), **kw)
    handle.session_gather(gather())
    st_neg = g["st"].copy()
    st_neg["A"][0] = -1
    for kw in (dict(offs=np.array([0, 256, 255], np.int64)), dict(st=st_neg), dict(regs=np.array([10, 266, 300, 300, 645, 901], np.int64)),
               dict(regs=np.array([-1, 255, 300, 300, 400, 656], np.int64)), dict(wav_ld=655), dict(rows=0), dict(wav_off=4),
               dict(operand=W.canary(g["rows"] * 160 + 417)), dict(operand=W.canary(g["rows"] * 160 + 415)), dict(n_ranges=np.array([-1], np.int32)),
               dict(wav=g["wav"][:g["wav_off"] + g["wav_ld"] - 1])):
        _refused(handle.session_gather, gather(**kw), f"gather: {sorted(kw)}")
    handle.session_gather(gather(wav_ld=656, wav=g["wav"][:g["wav_off"] + 656]))     # (the last sample read is the row's last)
    # ---- norm
    n = W.norm_cases()[0]
    norm = lambda **kw: dict(dict({k: n[k] for k in ("S", "n_mels", "mel_ld", "out_ld", "rows", "st", "mel")},
                                  out=W.canary(n["S"] * n["n_mels"] * n["out_ld"] + W.SLACK)), **kw)
    handle.session_norm(norm())
    for kw in (dict(rows=255), dict(mel_ld=n["rows"] - 1), dict(n_mels=0), dict(n_mels=129), dict(S=5), dict(out_ld=-1),
               dict(out=W.canary(n["S"] * n["n_mels"] * n["out_ld"] - 1)), dict(mel=n["mel"][:n["S"] * n["n_mels"] * n["mel_ld"] - 1])):
        _refused(handle.session_norm, norm(**kw), f"norm: {sorted(kw)}")
    # ---- session windows
    s = [s for s in W.session_window_cases() if s["name"] == "sw_64x7_J1_f160"][0]
    sw = lambda **kw: dict(_sw_job(s, W.session_windows_blank(s)), **kw)
    handle.session_windows(sw())                     # (accepted: a J above max_frames)
    assert max(s["st"]["J"]) > s["max_frames"]
    for kw in (dict(cap_windows=-(-s["max_frames"] // s["stride"]) - 1), dict(ld=s["width"] - 1), dict(max_frames=s["mel_ld"] + 1), dict(width=0),
               dict(stride=0), dict(n_mels=0), dict(n_mels=129), dict(win_off=8), dict(mel_off=4), dict(S=0),
               dict(mel=s["mel"][:s["mel_off"] + s["S"] * s["n_mels"] * s["mel_ld"] - 1]), dict(win=W.session_windows_blank(s)["win"][:100])):
        _refused(handle.session_windows, sw(**kw), f"session windows: {sorted(kw)}")
    # ---- stream windows
    items = [it for name, t in W.stream_tables() if name.startswith("geometry") for it in t]
    plain = [it for it in items if it["name"].startswith("wrap_J40_")][0]
    prov = [it for it in items if it["name"].startswith("seam_P5_")][0]
    call = lambda jobs: handle.stream_windows(jobs, W.canary_res(len(jobs)))
    mk = lambda it, **kw: [dict(_item_job(it, W.stream_out_blank(it)), **kw)]
    call(mk(plain)), call(mk(prov))
    for it, kw in ((plain, dict(width=0, n_frames=0)), (plain, dict(width=3001, ld=3001)), (plain, dict(n_frames=0)), (plain, dict(ld=plain["width"] - 1)),
                   (plain, dict(J=-1)), (plain, dict(n_frames=plain["width"] + 1)), (plain, dict(J=plain["n_frames"] - 1)),
                   (plain, dict(hist=plain["n_frames"] - 1)), (plain, dict(hist=0)), (plain, dict(n_mels=0)), (plain, dict(n_mels=129)),
                   (plain, dict(ring_off=4)), (plain, dict(out_off=8)), (plain, dict(fmax=plain["fmax"][:-1])),
                   (prov, dict(n_new=np.array([-1], np.int32))), (prov, dict(pv_ld=0)), (prov, dict(pv_off=4)),
                   (prov, dict(pvmax=prov["pvmax"][:-1])), (prov, dict(ring=prov["ring"][:prov["ring_off"] + prov["n_mels"] * prov["hist"] - 1]))):
        _refused(call, mk(it, **kw), f"stream windows: {sorted(kw)}")
    _refused(lambda jobs: handle.stream_windows(jobs, W.canary_res(1)), mk(plain) + mk(prov), "stream windows: res shorter than the table")
    _refused(call, mk(plain) * 65, "stream windows: 65 items")
    call(mk(prov, n_frames=prov["width"], hist=1, fmax=prov["fmax"][:1]))      # (accepted: hist = 1 with provisional frames)
