"""gemm_f32.hip, the slab depth as a property of the tile: with the weights as register fragments and
the fast epilogue, a 32-row tile takes 64-deep slabs and a 64- or 96-row tile 32-deep ones when the depth divides K, and 16 otherwise.
The MFMAs keep their order over k, so every launch must give gemm.hip's bits (layout 2), and the new staging map (thread ->
row, 16-byte piece of the row's part of the slab) must not change what a launch owns.  Bit equality and ownership only, through
css_gemm_host with kernel = 2; no float64 reference.  Each launch fills C and 128 rows of slack with the NaN canary of
tests/test_hip_gemm_epilogue.py and asserts

  ownership  every float outside {m < M, n < N} keeps the canary's bits;
  bits       C equals gemm.hip's result (layout 2) bit for bit.

K: 64 = one deep slab (the loop body never runs), 128 = the body once, 192 = both LDS buffers reused, 1824 = the embedding's K
(32 divides it, 64 does not: 57 slabs of 32 for heights 1 and 2).  css_gemm_host takes K % 32 == 0 only (tests/
test_hip_gemm_epilogue.py::test_refusals pins that), as every entry point of the library does, so a K that only 16 divides -- 16,
48, 80 -- cannot reach the kernel through it: those cases assert the refusal, and the fall-back to a shallower slab is walked by
the K that 32 divides and 64 does not: 32 (one slab, no loop), 96 and 160 (a 32-row tile falls back from 64 to 32).  So the
depth-16 bodies of heights 1 - 3 in the fragment kernel are not run by this file (nothing in the library reaches them).

Size: the tall shape is 6 K x 3 epilogues x 11 launches = 198 launches of 68 MB of C through the host and back, 0.6 s per K on
an MI355X box; the whole file (17 cases, 6 refusals among the launches) takes 5 s.  Needs an MI355X."""
import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

CANARY = 0x7FC0BEEF          # a quiet NaN with a payload (tests/test_hip_gemm_epilogue.py)
PREFIX = 64                  # floats in front of C
ACT_NONE, ACT_RELU = 0, 1
LAYOUTS = (0, 11, 12, 13, 14)   # the balanced plan; tiles of at most 1, 2, 3, 4 units
TALL = (4129, 4096)          # 130 row units x 32 panels = 4160 units over 1024 blocks: tiles of 2, 3 and 4 units in one launch
KMAX = 1824


@pytest.fixture(scope="module")
def handle():
    L = pkg("_lib")
    if L.load().css_device_count() < 1:
        pytest.fail("no HIP device visible")
    w = pkg("weights")
    desc = w.ModelDesc(num_blocks=1)
    sep = pkg("separator").HipSeparator(w.apply_golden_recipe(w.portable_state_dict(desc, 5)), None, device=0)
    yield sep.handle
    sep.close()


@pytest.fixture(scope="module")
def operands():
    """Seeded O(1) operands, made once: A [4129][1824], B [4096][1824], a column bias and a residual; a case takes the leading
    rows and the first K columns."""
    rng = np.random.default_rng(20261)
    m, n = TALL
    return dict(a=rng.standard_normal((m, KMAX), dtype=np.float32), b=rng.standard_normal((n, KMAX), dtype=np.float32),
                bias=rng.standard_normal(n, dtype=np.float32), res=rng.standard_normal((m, n), dtype=np.float32))


def _canary(n):
    return np.full(int(n), CANARY, np.uint32).view(np.float32)


EPILOGUES = {"none": dict(act=ACT_NONE, bias=False, residual=None, alpha=1.0),
             "relu": dict(act=ACT_RELU, bias=True, residual=None, alpha=1.0),
             "residual": dict(act=ACT_NONE, bias=True, residual="separate", alpha=0.5),
             "inplace": dict(act=ACT_NONE, bias=True, residual="inplace", alpha=0.5)}


class Case:
    """One (M, N, K, epilogue, ldc): the uploaded images are built once, every launch of the case reuses them."""

    def __init__(self, ops, m, n, k, epilogue, ldc=None):
        self.m, self.n, self.k, self.e = m, n, k, EPILOGUES[epilogue]
        self.ldc = n if ldc is None else ldc
        self.a = np.ascontiguousarray(ops["a"][:m, :k])
        self.b = np.ascontiguousarray(ops["b"][:n, :k])
        self.bias = np.ascontiguousarray(ops["bias"][:n]) if self.e["bias"] else None
        self.total = PREFIX + m * self.ldc + 128 * self.ldc
        self.c = _canary(self.total)
        self.residual = None
        if self.e["residual"] == "inplace":
            self.rows(self.c)[:, :n] = ops["res"][:m, :n]
            self.residual = "inplace"
        elif self.e["residual"] == "separate":
            self.residual = np.ascontiguousarray(ops["res"][:m, :n])

    def rows(self, flat):
        return flat[PREFIX:PREFIX + self.m * self.ldc].reshape(self.m, self.ldc)

    def launch(self, handle, what, **kw):
        out = handle.gemm(self.a, self.b, self.c, self.m, self.n, self.k, kernel=2, ldc=self.ldc, ldr=self.n, c_off=PREFIX,
                          act=self.e["act"], bias=self.bias, residual=self.residual, alpha=self.e["alpha"], **kw)
        bits = out.view(np.uint32)
        # ownership: in front of C, the ldc - N gap of every row, the 128 rows behind it
        assert (bits[:PREFIX] == CANARY).all(), (what, "written in front of C")
        assert (self.rows(bits)[:, self.n:] == CANARY).all(), (what, "written into the row gap")
        tail = bits[PREFIX + self.m * self.ldc:]
        stray = np.flatnonzero(tail != CANARY)
        assert stray.size == 0, (what, f"{stray.size} floats behind row M were written; the first at row {self.m + stray[0] // self.ldc}")
        y = self.rows(bits)[:, :self.n]
        assert (y != CANARY).all(), (what, "an owned float was left unwritten")
        return y

    def check(self, handle, what, layouts=LAYOUTS, frags=(True, False)):
        if self.k % 32:   # not a launch form of the library: refused, nothing launched
            with pytest.raises(pkg("_lib").CssError):
                self.launch(handle, (what, "refusal"), layout=0, b_frag32=True)
            return
        base = self.launch(handle, (what, "layout 2"), layout=2)
        for lay in layouts:
            for frag in frags:
                y = self.launch(handle, (what, lay, frag), layout=lay, b_frag32=frag)
                diff = np.flatnonzero((y != base).any(axis=1))
                assert diff.size == 0, (what, f"layout {lay}, b_frag32 {frag}", f"{diff.size} rows differ from gemm.hip; the first {diff[:4]}")


@pytest.mark.parametrize("k", [64, 128, 192, 48, 80, 96, 160, 1824])
def test_tall_launch_every_depth(handle, operands, k):
    """Tiles of 1 .. 4 units in one launch (balanced plan) and at each forced height, fragments on (deep slabs where the depth
    divides K) and off (16 deep throughout), for the three epilogues of the Linear layers."""
    m, n = TALL
    for epilogue in ("none", "relu", "residual"):
        Case(operands, m, n, k, epilogue).check(handle, (m, n, k, epilogue))


@pytest.mark.parametrize("n", [128, 256])
@pytest.mark.parametrize("m", [1, 31, 33, 97])
def test_rows_past_m(handle, operands, m, n):
    """The last tile's rows past M under the new staging map: they are read as zeros (the buffer descriptor's bound), never
    stored, and the rows below M keep their bits.  (K = 16: refused, see the module's text; K = 32: one slab of 32.)"""
    for k in (16, 32, 64, 128, 1824):
        Case(operands, m, n, k, "residual").check(handle, (m, n, k), frags=(True,))


def test_tall_launch_padded_rows_residual_in_place(handle, operands):
    """ldc = N + 4 and C = C + 0.5 (A B^T + bias): the 16-byte gap of every row stays untouched at every tile height."""
    m, n = TALL
    Case(operands, m, n, 128, "inplace", ldc=n + 4).check(handle, (m, n, 128, "ldc = N + 4, in place"), frags=(True,))
