"""Every launch form of mdhip_var (csrc/moments.hip: variance / std along one axis) and of plan_arg / run_arg (csrc/reduce.hip:
argmax / argmin along one axis) against exact references — the companion of tests/test_reduce_paths.py for the two reduction
families that module leaves out.

The centre is TABLE: what an entry reaches, the array it is cut from, the view taken, the reduced axis, the dtypes, the `edges`
(reduced indices on both sides of which the planted data sits), an optional option setting. There is no hook that reports which
kernel ran: every shape is derived from the launchers' predicates (MD_NUM_CUS 256, MD_BLOCK 256, MD_TICKET_WORDS 16384,
MD_TICKET_PAD 16; V = 16 bytes / element size; _nb_var / _nb_arg / _arg_chunk below repeat the launchers' arithmetic); the
`reaches` column is confirmed by a kernel trace of the gpu half (profiles/README.md: moments_arg_paths_kernel_stats.csv). The calls
go through the C-ABI (lib.var; lib.reduce with R_ARGMAX / R_ARGMIN) into a result block filled with a wrong value (85 / -7);
test_public_functions runs the same entries through nd.std / nd.argmax / nd.argmin with keepdims both ways.

Variance / std — bit for bit:
  data       per output x = m + d: m an integer, d integers in [-3, 3] that sum to 0 exactly (pairs +a, -a at random places); the
             edge positions carry distinct larger deviations in balanced fours (a, -(a+1), -(a+2), a+3; a = 10, 14, ..). m is as
             large as exactness allows (float32: n * (m + max|d| + 64) <= 2^24; float64: 2^30) and differs from output to output
             and from batch to batch. Every partial sum in any order is an exact integer, the mean is exactly m, every
             fma(d, d, q) is exact and q = sum d^2 is an exact integer (<= 2^22 in float32). Any E[x^2] - mean^2 formulation fails
             outright on such a mean.
  reference  q in int64, then T(q) / T(n - ddof), then np.sqrt if take_sqrt: the two correctly rounded operations the kernel does.
             ddof 0 and 1, take_sqrt 0 and 1 (the variance itself: no Python caller uses it).
  poison     a constant output gives exactly 0; an output owning one NaN, or one +inf, is NaN (as np.var / np.std say under
             np.errstate); every other output of those arrays keeps its bits (nothing leaks between rows, columns, batches).
  random     (the one inexact check) standard normals * 3 + 10 against np.longdouble, the bounds of tests/test_std_fused.py:
             relative 8 * 2e-6 (float32), 8 * 1e-13 (float64). The largest error / bound per entry goes to the file
             MDHIP_MOMENTS_PATHS_REPORT names (profiles/moments_paths_error.txt holds a device run's); the bound is not from it.
  sensitivity (host only) for every var entry and edge position a model of "this element dropped", "doubled" and "replaced by its
             neighbour" — the kernel's own two walks on the faulty data, in exact rational arithmetic — changes the reference.
  refusals   forms mdhip_var leaves to the caller raise ValueError and nd.std still gives NumPy's answer. More than 65535 batches
             over a middle axis (the smallest such operand is 2^30 elements): on the device alone, the operand built there from
             a (64, 256) slab of the exact data plus a per-batch integer; nd.std of it is exact on the composed route too.
The CPU double refuses a middle axis: that twin asserts the refusal and checks the integer reference against np.var in float64.

argmax / argmin — bit for bit against np.argmax / np.argmin of the same array: a permutation of distinct values per output (as
many as the type holds), and planted on it, each in an output of its own:
  the extreme at each edge position; the extreme twice, the second copy at a later index that the kernel merges EARLIER (a lower
  band, wave, lane or slot of the finish loop — the pairs are taken among the edge positions, which sit on both sides of every
  such boundary); floats: a NaN at an edge with a better value after it and a second NaN later, an extreme followed by a NaN (the
  NaN wins), all -inf, all +inf, all NaN, -0.0 with one +0.0, -inf (+inf) with one finite value; integers: the type's minimum and
  maximum as data, constant outputs of either (an all-identity column gives 0), int64 2^62 against 2^62 + 1 (equal as doubles),
  uint64 above 2^63 and uint32 above 2^31 against small values.
Column forms get their plants in the first and last column of a strip and the last V columns first, and some in every column at once.

Floats outside a view (padding of the base array) are NaN; integer padding is the value that would win the op under test (one base
array per op).

Each test has a twin: unmarked on the CPU double (skipped when a GPU is bound) — it proves that data and references are right —
and gpu-marked on the product library."""
import os
from fractions import Fraction

import numpy as np
import pytest

from minidiff_amd import _capi
from minidiff_amd import ndarray as nd

f16, f32, f64 = np.dtype(np.float16), np.dtype(np.float32), np.dtype(np.float64)
i8, i16, i32, i64 = np.dtype(np.int8), np.dtype(np.int16), np.dtype(np.int32), np.dtype(np.int64)
u8, u16, u32, u64 = np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.uint32), np.dtype(np.uint64)
b8 = np.dtype(np.bool_)
F, I = (f32, f64), (i32, i64)
N4 = F + I
S = slice

CODES = {"argmax": _capi.R_ARGMAX, "argmin": _capi.R_ARGMIN}
NP_ARG = {"argmax": np.argmax, "argmin": np.argmin}


def _vlen(dt):
    return max(1, 16 // dt.itemsize)


def _cdiv(a, b):
    return -(-a // b)


# ---- the launchers' arithmetic ----------------------------------------------------------------------------------------------------
def _nb_var(n, inner, outer, V):
    """Bands of k_var_cols (var_cols in moments.hip)."""
    NS = _cdiv(inner, 64 * V)
    NB = _cdiv(1024, NS) if outer == 1 else (1 if NS * outer >= 256 else 256 // (NS * outer))
    NB = max(1, min(NB, 64, n // 32))
    return 1 if NS * outer * 16 > 16384 else NB


def _nb_arg(n, inner, outer, V, blocks=256):
    """Bands of k_arg_cols_strips (argreduce in reduce.hip; blocks: option arg_blocks)."""
    NS = _cdiv(inner, 64 * V)
    NB = max(1, min(_cdiv(blocks, NS * outer), 64, n // 32))
    return 1 if outer > 1 and NS * outer * 16 > 16384 else NB


def _band_edges(n, NB, RB):
    """Row r of a strips walk lives in band r % NB, wave (r / NB) % 4, slot r / 4NB of its lane; RB slots make a batch. Boundaries:
    the second band, the second wave, a lane's second row, the second and third batch, the end of the whole batches (the row tail)."""
    step = 4 * NB
    cut = (n // (step * RB)) * step * RB
    return tuple(sorted({b for b in (NB, step, step * RB, 2 * step * RB, cut) if 1 <= b < n}))


def _arg_chunk(n_out, n_red, V):
    """(splits, chunk) of k_arg_rows_vec: ~2048 blocks, each with >= 8192 items of its row, chunks whole vectors."""
    splits = max(1, min(2048 // n_out, _cdiv(n_red, 8192)))
    chunk = _cdiv(_cdiv(n_red, splits), V) * V
    return _cdiv(n_red, chunk), chunk


assert _arg_chunk(2, 20000, 4) == (3, 6668) and _arg_chunk(3, 70000, 4) == (9, 7780) and _arg_chunk(3, 70000, 2) == (9, 7778)
assert _arg_chunk(1025, 8196, 4)[0] == 1 and _arg_chunk(3, 3076, 4)[0] == 1


def _mult(step, n, first=2, last=1):
    """A few of the multiples of `step` below n: the first ones and the last ones."""
    m = list(range(step, n, step))
    return tuple(sorted(set(m[:first] + m[-last:]))) if m else ()


def _apply_view(a, view, xp):
    """view: None | a tuple of slices | ("flip", axis) — the same cut of a NumPy array and of a DeviceArray."""
    if view is None:
        return a
    if view[0] == "flip":
        return xp.flip(a, view[1])
    return a[view]


class Entry:
    def __init__(self, id, reaches, base, axis, dtypes, view=None, edges=(), opt=None, family="arg", columns=False, middle=False, public_planted=False):
        self.id, self.reaches, self.base, self.axis, self.dtypes = id, reaches, tuple(base), axis, tuple(dtypes)
        self.view, self._edges, self.opt, self.family, self.columns, self.middle = view, edges, opt, family, columns, middle
        self.public_planted = public_planted
        self.shape = _apply_view(np.empty(self.base, dtype=np.bool_), view, np).shape
        self.axes = (axis,)
        self.kept = tuple(i for i in range(len(self.shape)) if i != axis)
        self.n_out = int(np.prod([self.shape[i] for i in self.kept], dtype=np.int64))
        self.n_red = self.shape[axis]
        self.inner = int(np.prod(self.shape[axis + 1:], dtype=np.int64))
        self.outer = int(np.prod(self.shape[:axis], dtype=np.int64))

    def edges(self, dt):
        return tuple(self._edges(dt)) if callable(self._edges) else tuple(self._edges)


VAR, ARG = [], []


def _var(id, *a, **k):
    VAR.append(Entry("var-" + id, *a, family="var", **k))


def _arg(id, *a, **k):
    ARG.append(Entry("arg-" + id, *a, **k))


# ---- mdhip_var, rows: the reduced axis contiguous, (rows, n), n % V == 0 ------------------------------------------------------------
# var_rows picks by vectors per row: <= 128 / 256 / 512 a wave per row caching 2 / 4 / 8 vectors per lane (four rows per block: row
# counts that are no multiple of 4 leave dead waves in the last block), <= 1024 / 4096 a block per row caching 4 / 16, longer rows
# are read twice (and need >= 256 rows). A thread takes vectors tig + g * G: the edges are the multiples of G * V elements.
_ROW_FORMS = ((1, "G=64 NV=2", 5), (128, "G=64 NV=2", 7), (129, "G=64 NV=4", 1), (256, "G=64 NV=4", 5), (257, "G=64 NV=8", 7),
              (512, "G=64 NV=8", 1), (513, "G=256 NV=4", 5), (1024, "G=256 NV=4", 7), (1025, "G=256 NV=16", 1), (4096, "G=256 NV=16", 5),
              (4097, "G=256 NV=0 (read twice)", 257))
for dt in F:
    for nvec, form, rows in _ROW_FORMS:
        n, G = nvec * _vlen(dt), 64 if nvec <= 512 else 256
        _var(f"rows-{dt.name}-{nvec}v", f"k_var_rows {form}", (rows, n), 1, (dt,), edges=_mult(G * _vlen(dt), n, first=99, last=0))
# many rows (an odd count: three dead waves at the end), and rows cut out of a NaN-padded base
_var("rows-1025x512", "k_var_rows G=64 NV=2 (float32) / NV=4 (float64), >= 1024 rows", (1025, 512), 1, F, edges=lambda dt: _mult(64 * _vlen(dt), 512, first=99, last=0))
_var("rows-padded-7x1040", "k_var_rows G=64 NV=8 (float32) / G=256 NV=4 (float64), rows 1 .. 7 of 9", (9, 1040), 1, F, view=(S(1, 8),),
     edges=lambda dt: _mult((64 if dt == f32 else 256) * _vlen(dt), 1040, first=99, last=0))


# ---- mdhip_var, columns: (n, inner) over axis 0 — the column sums of mdhip_reduce, then k_var_cols<T, 8> -----------------------------
def _var_col_edges(e):
    return lambda dt: _band_edges(e[0], _nb_var(e[0], e[1], e[2], _vlen(dt)), 8)


for shape, what, dts in (((64, 256), "NB 2, one batch of rows", F), ((67, 260), "NB 2, ragged last strip (clamped lanes), row tail", F),
                         ((4099, 256), "NB 64, two batches, with and without tail rows", F), ((6147, 256), "NB 64, three batches: the odd leftover", F),
                         ((64, 131072), "NB 1 (1024 strips): no partials, no ticket", (f64,))):
    _var("cols-%dx%d" % shape, f"k_var_cols 2-D, {what}", shape, 0, dts, columns=True, edges=_var_col_edges((shape[0], shape[1], 1)))
_var("cols-64x4x64", "k_var_cols 2-D, trailing axes collapse into inner = 256", (64, 4, 64), 0, F, columns=True, edges=_var_col_edges((64, 256, 1)))
_var("cols-1x128x512", "k_var_cols 2-D, a unit leading extent (SHAPES of test_middle_axis.py)", (1, 128, 512), 1, F, columns=True,
     edges=_var_col_edges((128, 512, 1)))
assert _nb_var(64, 256, 1, 4) == 2 and _nb_var(67, 260, 1, 4) == 2 and _nb_var(4099, 256, 1, 2) == 64 and _nb_var(64, 131072, 1, 2) == 1

# the batched launch: a middle axis, (outer, n, inner) — the SHAPES of test_middle_axis.py; NS * outer >= 256: NB 1, below: NB > 1
for shape, axis, what in (((2, 64, 256), 1, "NB 2"), ((3, 67, 260), 1, "NB 2, ragged strip, row tail"), ((5, 200, 512), 1, "NB 6, batches share the ticket block"),
                          ((300, 64, 256), 1, "NB 1"), ((2, 3, 64, 256), 2, "outer = 2 x 3"), ((2, 64, 4, 64), 1, "inner = 4 x 64")):
    _e = Entry("", "", shape, axis, F)
    _var("batched-" + "x".join(map(str, shape)), f"k_var_cols batched, {what}", shape, axis, F, columns=True, middle=True,
         edges=_var_col_edges((_e.n_red, _e.inner, _e.outer)))
assert _nb_var(200, 512, 5, 4) == 6 and _nb_var(64, 256, 300, 4) == 1 and _nb_var(64, 256, 2, 4) == 2


# ---- argreduce: k_arg_cols_strips<T, 4>, (n_red, n_out) over axis 0 ------------------------------------------------------------------
# n_out >= 256 whole vectors, 16-B rows, n_red >= 64, <= 1024 strips; NB = min(ceil(arg_blocks / NS), 64, n_red / 32); float32 / int32
# carry the row as 32 bits
def _arg_col_edges(n, inner, outer, blocks=(256,)):
    return lambda dt: tuple(sorted({b for k in blocks for b in _band_edges(n, _nb_arg(n, inner, outer, _vlen(dt), k), 4)}))


_arg("strips-64x256", "k_arg_cols_strips NB 2", (64, 256), 0, N4 + (u64,), columns=True, edges=_arg_col_edges(64, 256, 1))
_arg("strips-67x260", "k_arg_cols_strips NB 2, ragged last strip, row tail", (67, 260), 0, N4, columns=True, edges=_arg_col_edges(67, 260, 1))
_arg("strips-3075x256", "k_arg_cols_strips NB 64, three batches, tail", (3075, 256), 0, N4, columns=True, edges=_arg_col_edges(3075, 256, 1))
_arg("strips-window", "k_arg_cols_strips, row stride > n_out (an aligned column window)", (67, 520), 0, N4, view=(S(None), S(256, 516)), columns=True,
     edges=_arg_col_edges(67, 260, 1))
_arg("strips-nb-small", "k_arg_cols_strips NS 16, NB 1, 2, 3, 5 by option arg_blocks", (200, 4096), 0, (f32, i32), columns=True,
     edges=_arg_col_edges(200, 4096, 1, (16, 32, 48, 80)), opt=("arg_blocks", (16, 32, 48, 80)))
_arg("strips-nb1", "k_arg_cols_strips NS 256: NB 1 by itself", (64, 65536), 0, (f32,), columns=True, edges=_arg_col_edges(64, 65536, 1))
assert [_nb_arg(200, 4096, 1, 4, k) for k in (16, 32, 48, 80)] == [1, 2, 3, 5] and _nb_arg(64, 65536, 1, 4) == 1 and _nb_arg(3075, 256, 1, 2) == 64

# k_arg_cols_vec: 16 <= n_red < 64 (four rows in flight per wave: whole batches of 16 rows, then the `r += 4` tail), or more
# than 1024 strips
for n in (16, 17, 63):
    for c in (256, 260):
        _arg(f"colsvec-{n}x{c}", "k_arg_cols_vec, short columns", (n, c), 0, N4, columns=True, edges=(16, 48))
_arg("colsvec-1025-strips-f32", "k_arg_cols_vec, 1025 strips", (64, 262148), 0, (f32,), columns=True, edges=(16, 48))
_arg("colsvec-1025-strips-i64", "k_arg_cols_vec, 1025 strips", (64, 131074), 0, (i64,), columns=True, edges=(16, 48))

# the batched launch of the strips kernel: a middle axis (the SHAPES of test_middle_axis.py; (1,128,512) collapses to the 2-D form)
for shape, axis, what in (((2, 64, 256), 1, "NB 2"), ((3, 67, 260), 1, "NB 2, ragged strip, row tail"), ((5, 200, 512), 1, "NB 6"), ((300, 64, 256), 1, "NB 1"),
                          ((2, 3, 64, 256), 2, "outer = 2 x 3"), ((2, 64, 4, 64), 1, "inner = 4 x 64")):
    _e = Entry("", "", shape, axis, F)
    _arg("batched-" + "x".join(map(str, shape)), f"k_arg_cols_strips batched, {what}", shape, axis, N4 if shape[0] != 300 else (f32, i64), columns=True,
         edges=_arg_col_edges(_e.n_red, _e.inner, _e.outer))
_arg("batched-1x128x512", "k_arg_cols_strips 2-D (a unit leading extent)", (1, 128, 512), 1, F, columns=True, edges=_arg_col_edges(128, 512, 1))
_arg("batched-stride", "k_arg_cols_strips batched, batch stride > n_red * inner", (3, 70, 256), 1, N4, view=(S(None), S(3, 67)), columns=True,
     edges=_arg_col_edges(64, 256, 3))
assert _nb_arg(200, 512, 5, 4) == 6 and _nb_arg(64, 256, 300, 4) == 1

# k_arg_rows_vec FINAL: the reduced axis contiguous, n_red >= 1024, one chunk; a lane takes vectors tid, tid + 256 two at a time
_arg("rowsvec-1024", "k_arg_rows_vec FINAL, one vector per lane (float32)", (3, 1024), 1, N4, edges=lambda dt: _mult(256 * _vlen(dt), 1024))
_arg("rowsvec-2052", "k_arg_rows_vec FINAL, the two-vector loop", (3, 2052), 1, N4, edges=lambda dt: _mult(256 * _vlen(dt), 2052))
_arg("rowsvec-3076", "k_arg_rows_vec FINAL, the leftover vector", (3, 3076), 1, N4, edges=lambda dt: _mult(256 * _vlen(dt), 3076))
# (rows of 1029 cut to 1028: the three rows start 1, 2, 3 elements past 16 B — heads of 3, 2, 1 and tails of 1, 2, 3 float32)
_arg("rowsvec-head-tail", "k_arg_rows_vec FINAL, head peel and scalar tail", (3, 1029), 1, N4, view=(S(None), S(1, None)), edges=(4, 1024))
_arg("rowsvec-1025x8196", "k_arg_rows_vec FINAL, n_out > 1024 and n_red > 8192", (1025, 8196), 1, (f32,), edges=(1024, 2048, 8192))


# split: (2, 20000) 3 chunks of 6668 (last 6664); (3, 70000) 9 chunks of 7780 (float32 / int32) or 7778 (64-bit), last 7760 / 7776
def _chunk_edges(n_out, n_red):
    def f(dt):
        splits, chunk = _arg_chunk(n_out, n_red, _vlen(dt))
        assert splits > 1
        return (chunk, 2 * chunk, (splits - 1) * chunk)
    return f


_arg("rowsvec-split-2x20000", "k_arg_rows_vec split + k_arg_rows_finish (3 chunks)", (2, 20000), 1, N4, edges=_chunk_edges(2, 20000))
_arg("rowsvec-split-3x70000", "k_arg_rows_vec split + k_arg_rows_finish (9 chunks)", (3, 70000), 1, N4, edges=_chunk_edges(3, 70000))

# k_arg_rows_wave: a wave per row, 24 <= n_red <= 65536 (typed: < 1024), n_out >= 64; the lanes stride the row by 64
for n in (24, 63, 64, 65, 1023):
    _arg(f"wave-{n}", "k_arg_rows_wave typed", (64, n), 1, N4 + (u64,) if n == 65 else N4, edges=_mult(64, n))
_arg("wave-8200-rows", "k_arg_rows_wave typed, the wave loop past 8192 waves", (8200, 24), 1, (f32, i64))
_arg("wave-strided", "k_arg_rows_wave typed, strided row starts", (64, 100), 1, N4, view=(S(None), S(None, 65)), edges=(64,))
_NARROW = (b8, i8, u8, i16, u16, f16, u32)
_arg("wave-untyped-24", "k_arg_rows_wave untyped", (64, 24), 1, _NARROW)
_arg("wave-untyped-65536", "k_arg_rows_wave untyped, the longest row", (64, 65536), 1, _NARROW, edges=_mult(64, 65536))

# k_arg_block: n_red >= 512 that nothing above takes
_arg("block-10x600", "k_arg_block", (10, 600), 1, N4, edges=_mult(256, 600))
_arg("block-600x8", "k_arg_block, strided", (600, 8), 0, N4, edges=_mult(256, 600))
_arg("block-flipped", "k_arg_block, negative stride", (3, 1000), 1, N4, view=("flip", 1), edges=_mult(256, 1000))
_arg("block-i8-65537", "k_arg_block, untyped rows past the wave kernel", (2, 65537), 1, (i8,), edges=_mult(256, 65537))
_arg("block-misaligned", "k_arg_block, a misaligned column view", (600, 261), 0, N4, view=(S(None), S(1, None)), edges=_mult(256, 600))
_arg("block-u64", "k_arg_block, uint64 / uint32", (5, 700), 1, (u64, u32), edges=_mult(256, 700))

# k_arg_thread: everything else
for axis in (0, 1, 2):
    _arg(f"thread-5x7x9-{axis}", "k_arg_thread", (5, 7, 9), axis, N4 + (b8, u64, f16))
_arg("thread-1000x5", "k_arg_thread", (1000, 5), 1, N4)
_arg("thread-100x23", "k_arg_thread (one element short of the wave kernel)", (100, 23), 1, N4)
_arg("thread-one", "k_arg_thread, n_red == 1", (50, 1), 1, N4)
_arg("thread-misaligned", "k_arg_thread, a misaligned column view", (100, 261), 0, N4, view=(S(None), S(1, None)))

# lines that nd.argmax gathers into rows first (>= 16384 strided elements, <= 64 lines): test_public_functions runs every planted
# array of these two in every dtype (the edges are the chunks of the rows the gather makes: (2, 20000) 3 chunks, (6, 20000) 3 chunks);
# through the C-ABI the same arrays reach k_arg_block
_arg("gather-20000x2", "ndarray._arg_reduce: gather + k_arg_rows_vec split (C-ABI: k_arg_block)", (20000, 2), 0, (f32, i64), edges=_chunk_edges(2, 20000), public_planted=True)
_arg("gather-2x20000x3", "ndarray._arg_reduce: gather + k_arg_rows_vec split (C-ABI: k_arg_block)", (2, 20000, 3), 1, (f64, i32), edges=_chunk_edges(6, 20000), public_planted=True)

TABLE = VAR + ARG
BY_ID = {e.id: e for e in TABLE}
assert len(BY_ID) == len(TABLE)
assert max(int(np.prod(e.base)) for e in TABLE) <= 17 << 20


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def eager():
    prev = nd.set_lazy(False)
    yield
    nd.set_lazy(prev)


_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def error_report():
    yield
    path = os.environ.get("MDHIP_MOMENTS_PATHS_REPORT")
    if path and _RATIOS:
        with open(path, "w") as f:
            f.write("random float std of tests/test_moments_arg_paths.py: largest |got - longdouble| / |ref| per entry, as a fraction of the "
                    "asserted bound (8 * 2e-6 float32, 8 * 1e-13 float64)\n")
            for key in sorted(_RATIOS):
                f.write(f"{_RATIOS[key]:8.5f}  {key}\n")


def _twins(params):
    """Decorator: fn(case, mdopt, on_gpu) -> (CPU-double test, gpu-marked test), parametrised alike."""
    def deco(fn):
        @pytest.mark.parametrize("case", params)
        def cpu(lib, on_gpu, mdopt, case):
            if on_gpu:
                pytest.skip("other twin")
            fn(case, mdopt, False)

        @pytest.mark.gpu
        @pytest.mark.parametrize("case", params)
        def dev(lib, on_gpu, mdopt, case):
            assert on_gpu and lib.target == "hip:gfx950"
            fn(case, mdopt, True)
        return cpu, dev
    return deco


def _rng(e, dt, salt):
    return np.random.default_rng([TABLE.index(e), dt.num, salt])


def _from_rows(e, m):
    """(n_out, n_red) rows -> the logical array of the entry's view (outputs in C order of the kept axes)."""
    order = e.kept + e.axes
    v = m.reshape([e.shape[i] for i in order])
    return np.ascontiguousarray(v.transpose(np.argsort(order)))


def _upload(e, v, pad=None):
    """The logical array inside its base array (padding: NaN for floats, `pad` for integers) on the device, cut to the view. The
    caller keeps what it gets alive across the C call."""
    if e.view is None:
        return nd.asarray(v)
    base = np.full(e.base, np.nan if v.dtype.kind == "f" else pad, dtype=v.dtype)
    _apply_view(base, e.view, np)[...] = v
    return _apply_view(nd.asarray(base), e.view, nd)


def _equal(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    np.testing.assert_array_equal(got, ref, err_msg=str(what))      # (NaN equals NaN here; everything else bit for bit)


def _preferred_outputs(e, dt):
    """Column forms: the first and last column of the first two and the last strip and the last V columns, of the first and the
    last batch; then every output, spread evenly."""
    if not e.columns:
        return []
    V, inner = _vlen(dt), e.inner
    w = 64 * V
    last = ((inner - 1) // w) * w
    cols = [c for c in (0, w - 1, w, 2 * w - 1, last - 1, last) if 0 <= c < inner] + list(range(inner - V, inner))
    return list(dict.fromkeys([c for c in cols] + [e.n_out - inner + c for c in cols]))


def _deal(e, dt, items):
    """(output, item) pairs: every item gets an output of its own — the preferred ones first, then spread over the rest (the first
    and the last among them); with fewer outputs than items, several arrays."""
    n_out = e.n_out
    if n_out >= len(items):
        outs = _preferred_outputs(e, dt)[:len(items)]
        used, rest = set(outs), len(items) - len(outs)
        for k in range(rest):
            o = k * (n_out // rest) if k < rest - 1 else n_out - 1
            while o in used:
                o = (o + 1) % n_out
            used.add(o)
            outs.append(o)
        assert len(set(outs)) == len(items), (e.id, len(set(outs)), len(items))
        yield list(zip(outs, items))
        return
    for g in range(0, len(items), n_out):
        yield list(zip(range(n_out), items[g:g + n_out]))


# ---- variance: data -------------------------------------------------------------------------------------------------------------
def _var_positions(e, dt):
    """Edge positions of the reduced axis: both sides of every edge, the first and the last vector (rows) / the first four and last
    three (columns) — filled up to a multiple of four (the deviations there come in balanced fours)."""
    n, V = e.n_red, _vlen(dt)
    p = set(range(min(4, n))) | {n - 3, n - 2, n - 1}
    if not e.columns:
        p |= set(range(min(V, n))) | set(range(n - V, n))
    for edge in e.edges(dt):
        p |= {edge - 1, edge}
    p = sorted(q for q in p if 0 <= q < n)
    q = n // 2
    while len(p) % 4 and len(p) < n:
        if q not in p:
            p.append(q)
        q = (q + 1) % n
    p = sorted(p)
    return p[:len(p) // 4 * 4]


def _edge_devs(k):
    out = []
    for g in range(k // 4):
        a = 10 + 4 * g
        out += [a, -(a + 1), -(a + 2), a + 3]
    return np.array(out, dtype=np.int64)


def _var_data(e, dt, salt=1):
    """(x as rows (n_out, n), d as int64 rows, m per output as int64, edge positions)."""
    n, n_out = e.n_red, e.n_out
    rng = _rng(e, dt, salt)
    pos = _var_positions(e, dt)
    dev = _edge_devs(len(pos))
    L = n - len(pos)
    half = rng.integers(-3, 4, (n_out, L // 2))
    plain = rng.permuted(np.concatenate([half, -half, np.zeros((n_out, L % 2), dtype=np.int64)], axis=1), axis=1)
    d = np.empty((n_out, n), dtype=np.int64)
    mask = np.zeros(n, dtype=bool)
    mask[pos] = True
    d[:, mask] = dev
    d[:, ~mask] = plain
    assert (d.sum(axis=1) == 0).all()
    dmax = int(np.abs(dev).max(initial=3))
    top = (1 << 30) if dt == f64 else (1 << 24) // n - dmax - 64
    assert top >= 64, (e.id, dt.name, top)
    o = np.arange(n_out, dtype=np.int64)
    m = top - (o * 7) % 31 - 2 * ((o // e.inner) % 16)           # another mean in every output, another range in every batch
    q = (d * d).sum(axis=1)
    assert dt == f64 or (q.max() <= 1 << 22 and n * (int(m.max()) + dmax) <= 1 << 24)
    x = (m[:, None] + d).astype(dt)
    return x, d, m, pos


def _var_ref(e, q, dt, ddof, take_sqrt):
    """T(q) / T(n - ddof), then the square root: as rows (n_out,)."""
    r = q.astype(dt) / dt.type(e.n_red - ddof)
    assert r.dtype == dt
    return np.sqrt(r) if take_sqrt else r


def _kshape(e):
    return tuple(1 if i == e.axis else n for i, n in enumerate(e.shape))


def _var_direct(d, e, ddof, take_sqrt):
    res = nd.asarray(np.full(_kshape(e), 85, dtype=d.dtype))
    nd._lib().var(d.desc(), res.desc(), e.axis, ddof, take_sqrt)
    return res.get()


def _tol(dt):      # the bounds of test_std_fused.py / test_middle_axis.py for this kernel family
    return 8 * (2e-6 if dt == f32 else 1e-13)


def _check_var_entry(e, mdopt, on_gpu):
    refused = e.middle and not on_gpu                               # the double refuses a middle axis
    for dt in e.dtypes:
        x, d, m, pos = _var_data(e, dt)
        q = (d * d).sum(axis=1)
        v = _from_rows(e, x)
        dev = _upload(e, v)
        if refused:
            with pytest.raises(ValueError):
                _var_direct(dev, e, 0, 1)
            for ddof in (0, 1):
                np.testing.assert_allclose(q / (e.n_red - ddof), np.var(x.astype(np.float64), axis=1, ddof=ddof), rtol=1e-12)
            continue
        for ddof in (0, 1):
            for take_sqrt in (0, 1):
                ref = _var_ref(e, q, dt, ddof, take_sqrt).reshape(_kshape(e))
                _equal(_var_direct(dev, e, ddof, take_sqrt), ref, (e.id, dt.name, "exact", ddof, take_sqrt))
        # poison: a constant output, NaN / +inf in one place each of other outputs; the rest keeps its bits
        places = [pos[0], pos[len(pos) // 2], pos[-1]] if pos else [0, e.n_red - 1]
        for bad, take_sqrt in ((np.nan, 1), (np.inf, 0)):
            items = [("const", 0)] + [("bad", p) for p in dict.fromkeys(places)]
            for pairs in _deal(e, dt, items):
                xb = x.copy()
                ref = _var_ref(e, q, dt, 0, take_sqrt)
                for o, (kind, p) in pairs:
                    if kind == "const":
                        xb[o, :] = m[o]
                        ref[o] = 0
                    else:
                        xb[o, p] = bad
                        ref[o] = np.nan
                    with np.errstate(all="ignore"):
                        theirs = (np.std if take_sqrt else np.var)(xb[o])
                    assert theirs == 0 if kind == "const" else np.isnan(theirs), (e.id, kind, theirs)
                keep = _upload(e, _from_rows(e, xb))
                _equal(_var_direct(keep, e, 0, take_sqrt), ref.reshape(_kshape(e)), (e.id, dt.name, "poison", bad, pairs))
        # random data, the one inexact check
        h = (_rng(e, dt, 5).standard_normal(e.shape) * 3 + 10).astype(dt)
        keep = _upload(e, h)
        got = _var_direct(keep, e, 0, 1).astype(np.longdouble)
        ref = np.std(h.astype(np.longdouble), axis=e.axis, keepdims=True)
        ratio = float((np.abs(got - ref) / np.abs(ref)).max() / _tol(dt))
        _RATIOS[f"{e.reaches} [{e.id}, {dt.name}]"] = ratio
        assert ratio <= 1, (e.id, dt.name, ratio)


VAR_IDS = [e.id for e in VAR]
ARG_IDS = [e.id for e in ARG]


@_twins(VAR_IDS)
def _var_paths(case, mdopt, on_gpu):
    _check_var_entry(BY_ID[case], mdopt, on_gpu)


test_var_paths, test_var_paths_gpu = _var_paths


@pytest.mark.parametrize("case", VAR_IDS)
def test_var_data_is_sensitive(case):
    """Host only: the kernel's two walks (s = sum x, mean = s / n, q = sum (x - mean)^2) on data with one edge element dropped,
    doubled or replaced by a neighbour, in exact rational arithmetic (x = m + d with sum d = 0 gives closed forms), must change the
    reference in the type's own rounding — for every edge position, ddof 0 and 1."""
    e = BY_ID[case]
    for dt in e.dtypes:
        x, d, m, pos = _var_data(e, dt)
        n = e.n_red
        assert pos or n < 4
        for o in sorted({0, e.n_out - 1}):
            q = int((d[o] * d[o]).sum())
            mo = int(m[o])
            for p in pos:
                dp, xp = int(d[o, p]), mo + int(d[o, p])
                c = Fraction(xp, n)
                faults = {"dropped": q - dp * dp - 2 * c * dp + (n - 1) * c * c,          # mean' = m - c; the others move by +c
                          "doubled": q + n * c * c + (dp - c) ** 2}                       # mean' = m + c; one more term
                for nb in (p - 1, p + 1):
                    if 0 <= nb < n:
                        delta = int(d[o, nb]) - dp
                        faults[f"neighbour {nb}"] = q - dp * dp + int(d[o, nb]) ** 2 - Fraction(delta * delta, n)
                for ddof in (0, 1):
                    ref = dt.type(q) / dt.type(n - ddof)
                    for what, qf in faults.items():
                        bad = dt.type(float(qf)) / dt.type(n - ddof)
                        assert bad != ref and np.sqrt(bad) != np.sqrt(ref), (case, dt.name, o, p, what, float(qf), q)


# ---- variance: refusals ---------------------------------------------------------------------------------------------------------
def _refusals():
    rng = np.random.default_rng(71)

    def normal(shape, dt):
        return (rng.standard_normal(shape) * 3 + 10).astype(dt)

    yield "n % V != 0 (float32)", nd.asarray(normal((8, 1022), f32)), 1
    yield "n % V != 0 (float64)", nd.asarray(normal((8, 1023), f64)), 1
    yield "unaligned base", nd.asarray(normal((8 * 1024 + 4,), f32))[1:8 * 1024 + 1].reshape(8, 1024), 1
    yield "few long rows", nd.asarray(normal((255, 16388), f32)), 1
    yield "column form, n < 64", nd.asarray(normal((63, 256), f32)), 0
    yield "column form, inner < 256", nd.asarray(normal((64, 252), f32)), 0
    yield "column form, inner % V != 0", nd.asarray(normal((64, 258), f32)), 0


@_twins(["refusals"])
def _var_refusals(case, mdopt, on_gpu):
    """What mdhip_var leaves to the caller: ValueError from the C-ABI, NumPy's answer from nd.std (the composition's bounds:
    test_middle_axis.py). More than 65535 batches over a middle axis, device only (the double refuses every middle axis: the
    batched entries assert that): 65536 batches of one (64, 256) slab of the exact data, each raised by its own small integer on
    the device — std does not see the shift, and every sum of the composed passes is an exact integer, so NumPy's answer for the
    slab is the answer of every batch, bit for bit."""
    for what, d, axis in _refusals():
        assert d.is_c_contiguous, what
        kshape = tuple(1 if i == axis else n for i, n in enumerate(d.shape))
        res = nd.asarray(np.full(kshape, 85, dtype=d.dtype))
        with pytest.raises(ValueError):
            nd._lib().var(d.desc(), res.desc(), axis, 0, 1)
        assert (res.get() == 85).all(), what
        h = d.get()
        for ddof in (0, 1):
            got = nd.std(d, axis=axis, ddof=ddof)
            exp = np.std(h.astype(np.float64), axis=axis, ddof=ddof)
            assert got.dtype == h.dtype and got.shape == exp.shape, what
            np.testing.assert_allclose(got.get(), exp, rtol=2e-5 if h.dtype == f32 else 1e-12, err_msg=what)
    if not on_gpu:
        return
    e = BY_ID["var-cols-64x256"]
    x, d, m, pos = _var_data(e, f32, salt=9)
    slab = np.ascontiguousarray(x.T)                                # (64, 256); 64 below the exactness limit of the mean are free
    shift = (np.arange(65536) % 61).astype(f32).reshape(65536, 1, 1)
    big = nd.add(nd.asarray(slab.reshape(1, 64, 256)), nd.asarray(shift))
    assert big.shape == (65536, 64, 256) and big.dtype == f32 and big.is_c_contiguous
    res = nd.asarray(np.full((65536, 1, 256), 85, dtype=f32))
    with pytest.raises(ValueError):
        nd._lib().var(big.desc(), res.desc(), 1, 0, 1)
    assert (res.get() == 85).all()
    q = (d * d).sum(axis=1)
    for ddof in (0, 1):
        theirs = np.std(slab.astype(np.float64), axis=0, ddof=ddof)
        ref = _var_ref(e, q, f32, ddof, 1)
        np.testing.assert_allclose(ref, theirs, rtol=1e-6)
        got = nd.std(big, axis=1, ddof=ddof).get()
        _equal(got, np.ascontiguousarray(np.broadcast_to(ref, (65536, 256))), ("65536 batches", ddof))


test_var_refusals, test_var_refusals_gpu = _var_refusals


# ---- argmax / argmin: data --------------------------------------------------------------------------------------------------------
_SPAN = {i8: 200, u8: 190, f16: 2000, i16: 60000, u16: 60000}


def _extreme_rows(e, dt, rng):
    """Per output a permutation of distinct values (as many as the type holds); (rows, lowest - 7, highest + 7)."""
    span = min(e.n_red, _SPAN.get(dt, 1 << 62))
    off = 10 if dt.kind == "u" else -(span // 2)
    vals = np.arange(e.n_red, dtype=np.int64) % span + off
    m = rng.permuted(np.broadcast_to(vals, (e.n_out, e.n_red)), axis=1).astype(dt)
    return m, dt.type(off - 7), dt.type(off + span - 1 + 7)


def _arg_positions(e, dt):
    n, V = e.n_red, _vlen(dt)
    p = set(range(min(4, n))) | {V - 1, V, n // 2, (n // V) * V - 1, (n // V) * V - V, n - 3, n - 2, n - 1}
    for edge in e.edges(dt):
        p |= {edge - 1, edge, edge + 1}
    return sorted(q for q in p if 0 <= q < n)


def _arg_items(e, dt, pos, lo, hi):
    """Plants: (kind, positions ..). Every one is applied to an output of its own."""
    items = [(k, p) for p in pos for k in ("hi", "lo")]
    if e.n_out >= 200 and len(pos) > 1:           # many outputs: every pair among (at most 14 of) the edge positions
        key = pos if len(pos) <= 14 else sorted(set(pos[:5] + pos[-3:] + [q for ed in e.edges(dt)[:3] for q in (ed - 1, ed) if q in pos]))
        pairs = [(a, b) for i, a in enumerate(key) for b in key[i + 1:]]
    else:                                         # few: each position with the next, the third next and the last
        pairs = sorted({(a, pos[j]) for i, a in enumerate(pos) for j in (i + 1, i + 3, len(pos) - 1) if i < j < len(pos)})
    items += [(k, a, b) for a, b in pairs for k in ("hi2", "lo2")]
    some = list(dict.fromkeys([pos[0], pos[len(pos) // 2], pos[-1]]))
    if dt.kind == "f":
        for i, p in enumerate(pos):
            later = pos[i + 1:]
            if len(later) >= 2:
                items += [("nan-hi-nan", p, later[0], later[-1]), ("nan-lo-nan", p, later[0], later[-1])]
            if later:
                items += [("hi-nan", p, later[0]), ("lo-nan", p, later[-1])]
        items += [("row", -np.inf), ("row", np.inf), ("row", np.nan)]
        items += [(k, p) for p in some for k in ("zeros", "finite-", "finite+")]
    elif dt != b8:
        info = np.iinfo(dt)
        items += [("row", info.min), ("row", info.max)]
        items += [(k, p) for p in pos for k in ("tmin", "tmax")]
        items += [(k, p) for p in some for k in ("all-tmin-but", "all-tmax-but")]
        if dt == i64:
            items += [(k, p) for p in some for k in ("near+", "near-")]
        if dt in (u64, u32):
            items += [(k, p) for p in some for k in ("big", "small")]
    return items


def _plant(m, pairs, lo, hi):
    m = m.copy()
    dt = m.dtype
    for o, item in pairs:
        kind, a = item[0], item[1:]
        if kind in ("hi", "hi2"):
            m[o, list(a)] = hi
        elif kind in ("lo", "lo2"):
            m[o, list(a)] = lo
        elif kind in ("nan-hi-nan", "nan-lo-nan"):
            m[o, a[0]], m[o, a[1]], m[o, a[2]] = np.nan, hi if kind == "nan-hi-nan" else lo, np.nan
        elif kind in ("hi-nan", "lo-nan"):
            m[o, a[0]], m[o, a[1]] = hi if kind == "hi-nan" else lo, np.nan
        elif kind == "row":
            m[o, :] = a[0]
        elif kind == "zeros":
            m[o, :] = -0.0
            m[o, a[0]] = 0.0
        elif kind in ("finite-", "finite+"):
            m[o, :] = -np.inf if kind == "finite-" else np.inf
            m[o, a[0]] = 5.0
        elif kind == "tmin":
            m[o, a[0]] = np.iinfo(dt).min
        elif kind == "tmax":
            m[o, a[0]] = np.iinfo(dt).max
        elif kind == "all-tmin-but":
            m[o, :] = np.iinfo(dt).min
            m[o, a[0]] = np.iinfo(dt).min + 1
        elif kind == "all-tmax-but":
            m[o, :] = np.iinfo(dt).max
            m[o, a[0]] = np.iinfo(dt).max - 1
        elif kind in ("near+", "near-"):                            # equal once rounded to a double
            m[o, :] = (1 << 62) + (kind == "near-")
            m[o, a[0]] = (1 << 62) + (kind == "near+")
        elif kind in ("big", "small"):                              # negative if read as the signed type
            top = dt.type(1) << dt.type(8 * dt.itemsize - 1)
            if kind == "big":
                m[o, a[0]] = top + dt.type(5)
            else:
                m[o, :] = top + dt.type(7)
                m[o, a[0]] = 3
        else:
            raise AssertionError(kind)
    return m


def _arg_variants(e, dt, planted):
    """[(what, rows)]: the permutation, then the planted arrays."""
    rng = _rng(e, dt, 3)
    if dt == b8:                                                    # two values: one True among False, one False among True
        pos = _arg_positions(e, dt)
        out = []
        for fill in (False, True):
            rows0 = np.full((e.n_out, e.n_red), fill, dtype=dt)
            out.append((f"all {fill}", rows0))
            if planted:
                items = [("lo" if fill else "hi", p) for p in pos] + [("lo2" if fill else "hi2", a, b) for a, b in zip(pos, pos[1:])]
                out += [(f"planted {pairs[:2]} ..", _plant(rows0, pairs, False, True)) for pairs in _deal(e, dt, items)]
        return out
    m, lo, hi = _extreme_rows(e, dt, rng)
    out = [("permutation", m)]
    if not planted:
        return out
    pos = _arg_positions(e, dt)
    items = _arg_items(e, dt, pos, lo, hi)
    out += [(f"planted {pairs[:2]} ..", _plant(m, pairs, lo, hi)) for pairs in _deal(e, dt, items)]
    if e.columns and len(pos) > 4 and e.n_out * e.n_red <= 1 << 21:                                  # in every column at once (the clamped lanes of a ragged strip too)
        every = slice(None)
        out.append(("hi in the last row, every column", _plant(m, [(every, ("hi", pos[-1]))], lo, hi)))
        out.append(("lo in the last row, every column", _plant(m, [(every, ("lo", pos[-1]))], lo, hi)))
        out.append(("twice, every column", _plant(m, [(every, ("hi2", pos[1], pos[-2])), (every, ("lo2", pos[2], pos[-1]))], lo, hi)))
    return out


def _arg_direct(op, d, e):
    res = nd.asarray(np.full(_kshape(e), -7, dtype=np.int64))
    nd._lib().reduce(CODES[op], d.desc(), res.desc(), 1 << e.axis)
    return res.get()


def _pad(op, dt):
    if dt.kind == "f":
        return None
    if dt == b8:
        return op == "argmax"
    info = np.iinfo(dt)
    return info.max if op == "argmax" else info.min


def _check_arg_entry(e, mdopt, on_gpu, public=False, dtypes=None, planted=True):
    opt_values = e.opt[1] if e.opt else (None,)
    if not on_gpu:
        opt_values = opt_values[:1]                                 # (the double has one loop: the option changes nothing)
    for dt in dtypes or e.dtypes:
        runs = []                                                   # (what, {op: device array}, host array)
        for what, rows in _arg_variants(e, dt, planted=planted):
            v = _from_rows(e, rows)
            if e.view is None or dt.kind == "f":
                d = _upload(e, v)
                dev = {"argmax": d, "argmin": d}
            else:
                dev = {op: _upload(e, v, _pad(op, dt)) for op in CODES}
            runs.append((what, dev, v))
        for value in opt_values:
            if value is not None:
                mdopt(e.opt[0], value)
            for what, dev, v in runs:
                for op in CODES:
                    ref = NP_ARG[op](v, axis=e.axis, keepdims=True)
                    if public:
                        for keep in (True, False):
                            got = getattr(nd, op)(dev[op], axis=e.axis, keepdims=keep).get()
                            _equal(got, ref if keep else ref.squeeze(e.axis), (e.id, dt.name, op, what, keep))
                    else:
                        _equal(_arg_direct(op, dev[op], e), ref, (e.id, dt.name, op, what, value))


@_twins(ARG_IDS)
def _arg_paths(case, mdopt, on_gpu):
    _check_arg_entry(BY_ID[case], mdopt, on_gpu)


test_arg_paths, test_arg_paths_gpu = _arg_paths


# ---- the public functions ---------------------------------------------------------------------------------------------------------
@_twins([e.id for e in TABLE])
def _public_functions(case, mdopt, on_gpu):
    """The same entries through nd.std / nd.argmax / nd.argmin, keepdims both ways (first dtype; arg: the permutation alone — but the lines nd.argmax gathers into rows: everything). std of
    the exact data is exact on every route: the composed passes (the double over a middle axis) meet the same integers."""
    e = BY_ID[case]
    if e.family == "arg":
        _check_arg_entry(e, mdopt, on_gpu, public=True, dtypes=e.dtypes if e.public_planted else e.dtypes[:1], planted=e.public_planted)
        return
    dt = e.dtypes[0]
    x, d, m, pos = _var_data(e, dt, salt=2)
    q = (d * d).sum(axis=1)
    dev = _upload(e, _from_rows(e, x))
    for ddof in (0, 1):
        ref = _var_ref(e, q, dt, ddof, 1).reshape(_kshape(e))
        for keep in (True, False):
            got = nd.std(dev, axis=e.axis, ddof=ddof, keepdims=keep).get()
            _equal(got, ref if keep else ref.squeeze(e.axis), (e.id, dt.name, ddof, keep))


test_public_functions, test_public_functions_gpu = _public_functions
