"""Every launch form of the plain reductions (csrc/reduce.hip, plan_reduce / run_reduce: sum, prod, max, min, any / all over an
axis) against exact references.

The centre is TABLE: what an entry reaches, the array it is cut from, the view taken, the reduced axes, the dtypes. There is no
hook that reports which kernel ran: every shape is derived from the planner's predicates (plan_reduce, whose tests stand in the
order of the route; MD_NUM_CUS 256, MD_BLOCK 256,
MD_TICKET_WORDS 16384, MD_TICKET_PAD 16; V = 16 bytes / element size); the `reaches` column is to be confirmed by a kernel trace of
the gpu half (profiles/README.md: reduce_paths_kernel_stats.csv). The calls go through the C-ABI as ndarray._reduce does at its end
(DeviceArray.empty + lib.reduce), so that neither _staged_reduce nor lazy fusion re-expresses them; test_public_functions runs
the same entries through nd.sum / nd.prod / nd.max / nd.min / nd.any / nd.all.

Data and references — every check is bit for bit, except the one marked:
  sum, floats    odd integers of either sign, magnitude <= min(1001, (2^24 - 1) // n_red) (float32) or 1001 (float64): every
                 partial sum in every order is an exact integer, so the result equals NumPy's int64 sum; a dropped, doubled or
                 misplaced element (an odd number) changes it.
  sum, integers  full-range random values: the wrap-around must be NumPy's (storage-only inputs: NumPy's int64 / uint64 loop).
  prod, floats   per output at most 100 twos and 100 halves at random places, -1 everywhere else: every partial product in any
                 order lies within 2^+-100 (exact in both float types); a dropped element changes the sign or the magnitude.
  prod, integers full-range random ODD values other than +-1: odd numbers are units modulo 2^64, so every factor counts (with
                 even factors the product of a few dozen elements is 0 whatever else happens).
  max / min      a permutation of distinct values per output, then the extreme planted at reduced index 0 .. 3, V - 1, in the
                 last whole vector, in the scalar tail and on both sides of every chunk / band / wave boundary of the entry
                 (`edges`); floats: a NaN at each of those places (the output that owns it is NaN, NumPy's max / min of the same
                 array says what every other output is) and an all -inf and an all +inf output.
  any / all      one true among zeros, one zero among ones, at the same places.
  sum, random    (the one inexact check) standard normals * 3 + 10 against np.longdouble:
                 |got - ref| <= min(n_red - 1, 34) * u * sum|x|, u = 2^-24 / 2^-53. n_red - 1 is the worst case of ANY summation
                 order; 34 u is the bound test_large_shape_paths._staged has always used for float32 (2e-6), in unit roundoffs,
                 carried to float64. The largest observed ratio per path is written to the file MDHIP_REDUCE_PATHS_REPORT names
                 (profiles/reduce_paths_error.txt is meant to hold the device run's); the bound does not come from it.
Floats outside a view (padding of the base array) are NaN, integers random: a kernel that folds an element from outside its
view fails the exact checks. The result block is filled with a wrong value before the call: an output that is never written
does not pass on what the allocator's previous user left there.

Each test has a twin: unmarked on the CPU double (skipped when a GPU is bound) — it proves that data and references are right —
and gpu-marked on the product library."""
import os

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

CODES = {"sum": _capi.R_SUM, "prod": _capi.R_PROD, "max": _capi.R_MAX, "min": _capi.R_MIN, "any": _capi.R_ANY, "all": _capi.R_ALL}
S = slice


class Entry:
    def __init__(self, id, reaches, base, axes, dtypes, view=None, ops=None, edges=(), opt=None, ticket=False):
        self.id, self.reaches, self.base, self.axes, self.dtypes = id, reaches, tuple(base), tuple(sorted(axes)), tuple(dtypes)
        self.view, self.ops, self.edges, self.opt, self.ticket = view, ops, tuple(edges), opt, ticket
        self.shape = _apply_view(np.empty(self.base, dtype=np.bool_), view, np).shape
        self.kept = tuple(i for i in range(len(self.shape)) if i not in self.axes)
        self.n_out = int(np.prod([self.shape[i] for i in self.kept], dtype=np.int64))
        self.n_red = int(np.prod([self.shape[i] for i in self.axes], dtype=np.int64))

    def ops_for(self, dt):
        if self.ops is not None:
            return self.ops
        if dt == b8:
            return ("any", "all")
        if dt.kind == "f":
            return ("sum", "prod", "max", "min", "rand")
        return ("sum", "prod", "max", "min")


def _apply_view(a, view, xp):
    """view: None | a tuple of slices | ("flip", axis) — the same cut of a NumPy array and of a DeviceArray."""
    if view is None:
        return a
    if view[0] == "flip":
        return xp.flip(a, view[1])
    return a[view]


def _mult(step, n, first=2, last=1):
    """A few of the multiples of `step` below n: the first ones and the last ones."""
    m = list(range(step, n, step))
    return tuple(sorted(set(m[:first] + m[-last:]))) if m else ()


TABLE = []


def _add(*a, **k):
    TABLE.append(Entry(*a, **k))


# ---- rows: the reduced axis contiguous, (n_out, n_red), axis 1 ----------------------------------------------------------------
# k_reduce_rows_wave<NV>: n_out >= 1024, 32 <= n_red <= 64 * V * 8, every row on 16 B; NV by n_red // V: <= 64, 128, 256, 512.
# A lane takes vectors lane + 64 g: the edges are the multiples of 64 * V elements.
for n, nv in ((32, 1), (256, 1), (260, 2), (512, 2), (516, 4), (1024, 4), (1028, 8), (2048, 8)):
    _add(f"wave-f32-{n}", f"k_reduce_rows_wave NV={nv}", (1024, n), (1,), (f32, i32) if n in (260, 2048) else (f32,), edges=_mult(256, n))
for n, nv in ((32, 1), (128, 1), (130, 2), (256, 2), (258, 4), (512, 4), (514, 8), (1024, 8)):
    _add(f"wave-f64-{n}", f"k_reduce_rows_wave NV={nv}", (1024, n), (1,), (f64, i64) if n in (130, 1024) else (f64,), edges=_mult(128, n))
# n_red % V != 0 needs padded rows (every row starts on 16 B): a view of wider rows
_add("wave-tail-255", "k_reduce_rows_wave, scalar tail (f32 NV=1, f64 NV=2)", (1024, 264), (1,), N4, view=(S(None), S(None, 255)), edges=(128,))
_add("wave-tail-2047", "k_reduce_rows_wave NV=8, scalar tail", (1024, 2052), (1,), (f32, i32), view=(S(None), S(None, 2047)), edges=_mult(256, 2047))
_add("wave-tail-1023", "k_reduce_rows_wave NV=8, scalar tail", (1024, 1026), (1,), (f64, i64), view=(S(None), S(None, 1023)), edges=_mult(128, 1023))
# one vector past the range: a block per row
_add("wave-past-2052", "k_reduce_rows mode 0 (n_red one vector past the wave kernel)", (1024, 2052), (1,), (f32,), edges=_mult(1024, 2052))

# k_reduce_rows_wave_any: 16 <= n_red <= 4096, n_out >= 256, not (typed and n_red >= 256); lanes stride the row by 64
_add("waveany-i8", "k_reduce_rows_wave_any, int8 -> int64", (256, 4096), (1,), (i8,), ops=("sum",), edges=_mult(64, 4096))
_add("waveany-bool", "k_reduce_rows_wave_any, 1-byte accumulator", (256, 17), (1,), (b8,))
_add("waveany-f16", "k_reduce_rows_wave_any, float16 -> float", (256, 100), (1,), (f16,), ops=("sum", "max", "min"), edges=(64,))
_add("waveany-short", "k_reduce_rows_wave_any, typed, under 1024 rows", (256, 37), (1,), N4)
_add("waveany-misaligned", "k_reduce_rows_wave_any, rows off 16 B", (1024, 251), (1,), N4, view=(S(None), S(1, None)), edges=(64, 128, 192))

# k_reduce_rows mode 0: one block per output. Vector form: item lane0 of 256 lanes, four / two / one loads in flight
_add("rows-256", "k_reduce_rows mode 0", (3, 256), (1,), N4)
_add("rows-1000", "k_reduce_rows mode 0", (3, 1000), (1,), N4)
_add("rows-head-1003", "k_reduce_rows mode 0, head peel", (3, 1004), (1,), N4, view=(S(None), S(1, None)))
# (rows of 1005 cut to 1004: the three rows start 1, 2, 3 elements past 16 B — heads of 3, 2, 1 and tails of 1, 2, 3 float32)
_add("rows-head-tail-1004", "k_reduce_rows mode 0, head peel and scalar tail", (3, 1005), (1,), N4, view=(S(None), S(1, None)))
_add("rows-long-4100", "k_reduce_rows mode 0, four loads in flight, then one", (600, 4100), (1,), (f32,), edges=(1024, 4096), ops=("sum", "max", "min"))
_add("rows-strided", "k_reduce_rows mode 0, one strided reduced axis", (300, 8), (0,), N4, edges=(256,))
_add("rows-two-axes", "k_reduce_rows mode 0, two reduced axes", (20, 3, 20), (0, 2), N4, edges=(256,))
_add("rows-flipped", "k_reduce_rows mode 0, negative stride", (3, 1000), (1,), N4, view=("flip", 1), edges=(256, 512))

# k_reduce_rows mode 2: `splits` blocks per row sweep it together (item s * 256 + tid, step splits * 256), partials + ticket
_add("ticket-5", "k_reduce_rows mode 2, md_ticket_last (5 splits)", (4, 20000), (1,), N4, edges=(1024, 1280, 5120, 19456), ticket=True)
_add("ticket-65", "k_reduce_rows mode 2, md_ticket_last2 (65 splits)", (2, 262149), (1,), N4, edges=(1024, 66560, 133120, 261120), ticket=True)
_add("ticket-misaligned", "k_reduce_rows mode 2, n_out 1, base off 16 B", (20001,), (0,), N4, view=(S(1, None),), edges=_mult(1024, 20000), ticket=True)
# 1-byte accumulators: partials + k_finish_rows
_add("finish-rows-bool", "k_reduce_rows mode 1 + k_finish_rows", (3, 10000), (1,), (b8,), edges=_mult(256, 10000))

# k_reduce_all: the whole of an aligned contiguous array; vectors gid, gid + grid; 2 / 5 / 64 blocks (64: two-level ticket)
for n in (4097, 20003, 258053):
    _add(f"all-{n}", f"k_reduce_all ({-(-n // 4096)} blocks)", (n,), (0,), N4, edges=(512, 1024, 4096) + _mult(1024, n)[-1:], ticket=True)
_add("all-narrow-sum", "k_reduce_all, storage-only -> int64", (20003,), (0,), (i8, i16, u8, u16, u32, u64), ops=("sum", "prod"), edges=_mult(4096, 20003), ticket=True)
_add("all-narrow-max-i32", "k_reduce_all, storage-only, int32 carrier", (20003,), (0,), (i8, i16, u8, u16), ops=("max", "min"), edges=_mult(4096, 20003))
_add("all-narrow-max-i64", "k_reduce_all, uint32, int64 carrier", (20003,), (0,), (u32,), ops=("max", "min"), edges=_mult(4096, 20003))
_add("all-f16", "k_reduce_all, float16, float carrier", (20003,), (0,), (f16,), ops=("sum", "max", "min"), edges=_mult(4096, 20003))

# ---- columns: the kept axis contiguous, (n_red, n_out), axis 0 -----------------------------------------------------------------
# k_reduce_cols_strips (sum, prod; float32 max / min): n_red >= 512, NS = ceil(n_out / 64 V) strips x NB bands >= 64 blocks,
# NB = min(256 / NS, 64, n_red / 32); row = band + NB * (wave + 4 i): neighbouring rows belong to different bands / waves
_add("strips-512x1024", "k_reduce_cols_strips NS 4, NB 16", (512, 1024), (0,), (f32, i32), edges=(16, 64, 256), ticket=True)
_add("strips-517x1028", "k_reduce_cols_strips NS 5, NB 16, ragged last strip, row tail", (517, 1028), (0,), (f32, i32), edges=(16, 64, 512), ticket=True)
_add("strips-2048x256", "k_reduce_cols_strips NS 1, NB 64", (2048, 256), (0,), (f32, i32), edges=(64, 256, 1024), ticket=True)
_add("strips-64bit", "k_reduce_cols_strips, V = 2", (512, 512), (0,), (f64, i64), edges=(16, 64, 256), ops=("sum", "prod", "rand"), ticket=True)
# option cols_nb forces the band count; with NS * NB >= 64 still to hold, NB 1 .. 5 need 64 strips: 16384 float32 columns
# (NB 1: no partial rows, no ticket; 2, 3, 5: even and odd band counts, bands per merging wave 1 and 2; 64: 16 per wave)
_add("strips-nb-small", "k_reduce_cols_strips NS 64, NB 1, 2, 3, 5 by option", (512, 16384), (0,), (f32,), ops=("sum", "max"), edges=(5, 6, 32),
     opt=("cols_nb", (1, 2, 3, 5)))
_add("strips-nb-64", "k_reduce_cols_strips NS 4, NB 64 by option", (2048, 1024), (0,), (f32,), edges=(64, 256, 1024), opt=("cols_nb", (64,)))

# the batched launch of the strips kernel: a middle axis, (outer, n_red, inner), inner >= 256, n_red >= 64
_add("batched-2x64x256", "k_reduce_cols_strips batched, NB 2", (2, 64, 256), (1,), F, edges=(2, 8, 32), ticket=True)
_add("batched-3x67x260", "k_reduce_cols_strips batched, ragged strip, row tail", (3, 67, 260), (1,), F, edges=(2, 8, 64), ticket=True)
_add("batched-5x200x512", "k_reduce_cols_strips batched, NB 6", (5, 200, 512), (1,), F, edges=(6, 24, 192), ticket=True)
_add("batched-300x64x256", "k_reduce_cols_strips batched, NB 1", (300, 64, 256), (1,), F, edges=(4, 32))
_add("batched-2x3x64x256", "k_reduce_cols_strips batched, outer = 2 x 3", (2, 3, 64, 256), (2,), F, edges=(2, 8, 32), ticket=True)

# k_reduce_cols_vec: 64 lanes x one 16-B vector of columns, four row lanes, chunks of rows in gridDim.y (a multiple of 16 rows)
_add("vec-100x256", "k_reduce_cols_vec FINAL", (100, 256), (0,), N4, edges=(16, 96))
_add("vec-300x256", "k_reduce_cols_vec non-FINAL + FINAL (4 chunks of 80)", (300, 256), (0,), N4, edges=(80, 160, 240))
_add("vec-1000x260", "k_reduce_cols_vec non-FINAL + FINAL (13 chunks of 80; float64 / int64 sum, prod: strips)", (1000, 260), (0,), N4, edges=(80, 160, 960))
_add("vec-maxmin", "k_reduce_cols_vec: float64 / integer max and min stay off the strips kernel", (600, 512), (0,), (f64, i32, i64), ops=("max", "min"),
     edges=(80, 160, 560))

# k_reduce_cols: a lane per column, chunks of rows in gridDim.y
_add("cols-40x67", "k_reduce_cols FINAL", (40, 67), (0,), N4, edges=(36,))
_add("cols-300x67", "k_reduce_cols non-FINAL + k_finish_cols (9 chunks of 34)", (300, 67), (0,), N4, edges=(34, 68, 272))
_add("cols-i8", "k_reduce_cols + k_finish_cols, int8 -> int64", (300, 256), (0,), (i8,), ops=("sum",), edges=(34, 272))
_add("cols-two-axes", "k_reduce_cols + k_finish_cols, two reduced axes (2 chunks of 40)", (10, 15, 67), (0, 1), N4, view=(S(None), S(None, None, 2)), edges=(40,))
_add("cols-bool", "k_reduce_cols + k_finish_cols, 1-byte accumulator", (300, 256), (0,), (b8,), edges=(34, 68, 272))
_add("cols-middle-f64", "k_reduce_cols: float64 / integer max and min over a middle axis", (3, 67, 260), (1,), (f64, i32), ops=("max", "min"), edges=(34,))

# k_reduce_generic: everything else
for axes in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):
    _add("generic-" + "".join(map(str, axes)), "k_reduce_generic", (5, 7, 9), axes, N4 + (b8,))

BY_ID = {e.id: e for e in TABLE}
assert len(BY_ID) == len(TABLE)


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
    path = os.environ.get("MDHIP_REDUCE_PATHS_REPORT")
    if path and _RATIOS:
        with open(path, "w") as f:
            f.write("random float sums of tests/test_reduce_paths.py: largest |got - longdouble| / (u * sum|x|) per path (bound: min(n_red - 1, 34))\n")
            for key in sorted(_RATIOS):
                f.write(f"{_RATIOS[key]:8.3f}  {key}\n")


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


def _out_dtype(op, dt):
    if op in ("any", "all"):
        return b8
    if op in ("max", "min"):
        return dt
    if dt == f16:
        return f32                      # the float carrier itself: exact integer sums
    if dt in (i32, i64, f32, f64):
        return dt                       # the typed kernels (int32 sums wrap in int32, as np.sum(dtype=int32))
    return nd._sum_dtype(dt, None)      # storage-only integers: int64 / uint64


def _poison(op, dt):
    if dt == b8:
        return op == "any"              # most outputs of the any cases are False, of the all cases True
    return 85


def _direct(op, d, axes, odt):
    mask = 0
    for ax in axes:
        mask |= 1 << ax
    kshape = tuple(1 if (mask >> i) & 1 else n for i, n in enumerate(d.shape))
    res = nd.asarray(np.full(kshape, _poison(op, odt), dtype=odt))
    nd._lib().reduce(CODES[op], d.desc(), res.desc(), mask)
    return res.get()


def _public(op, d, axes, odt):
    kw = {"dtype": odt} if op in ("sum", "prod") else {}
    return getattr(nd, op)(d, axis=axes, keepdims=True, **kw).get()


def _rng(e, dt, salt):
    return np.random.default_rng([TABLE.index(e), dt.num, salt])


def _from_rows(e, m):
    """(n_out, n_red) rows -> the logical array of the entry's view: reduced index r walks the reduced axes in C order."""
    order = e.kept + e.axes
    v = m.reshape([e.shape[i] for i in order])
    return np.ascontiguousarray(v.transpose(np.argsort(order))) if order else v.reshape(e.shape)


def _upload(e, v, rng):
    """The logical array inside its base array (NaN / random padding) on the device, cut to the view."""
    if e.view is None:
        return nd.asarray(v)
    dt = v.dtype
    if dt.kind == "f":
        base = np.full(e.base, np.nan, dtype=dt)
    elif dt == b8:
        base = rng.integers(0, 2, e.base).astype(dt)
    else:
        info = np.iinfo(dt)
        base = rng.integers(info.min, info.max, e.base, dtype=dt, endpoint=True)
    _apply_view(base, e.view, np)[...] = v
    return _apply_view(nd.asarray(base), e.view, nd)


def _positions(e, dt):
    n, V = e.n_red, max(1, 16 // dt.itemsize)
    p = set(range(min(4, n))) | {V - 1, n // 2, (n // V) * V - 1, (n // V) * V - V, n - 2, n - 1}
    for edge in e.edges:
        p |= {edge - 1, edge}
    return sorted(q for q in p if 0 <= q < n)


def _groups(e, items):
    """Deal (output, item) pairs: every item gets an output of its own, spread over the outputs (the first and the last among
    them); with fewer outputs than items, several arrays."""
    n_out = e.n_out
    if n_out >= len(items):
        step = n_out // len(items)
        outs = [k * step for k in range(len(items))]
        outs[-1] = n_out - 1
        yield list(zip(outs, items))
        return
    for g in range(0, len(items), n_out):
        yield list(zip(range(n_out), items[g:g + n_out]))


# ---- data -----------------------------------------------------------------------------------------------------------------------
def _sum_rows(e, dt, rng):
    shape = (e.n_out, e.n_red)
    if dt.kind == "f":
        mag = 1001
        if dt == f32 or dt == f16:
            mag = min(1001, (2 ** 24 - 1) // max(e.n_red, 1))
        half = (mag + 1) // 2                                   # odd magnitudes 1, 3, .. <= mag
        m = 2 * rng.integers(0, half, shape) + 1
        return (m * rng.choice((-1, 1), shape)).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)


def _sum_ref(v, axes, dt, odt):
    if dt.kind == "f":
        r = v.astype(np.int64).sum(axis=axes, keepdims=True)
        assert dt == f64 or np.abs(r).max(initial=0) < 2 ** 24
        return r.astype(odt)
    return np.sum(v, axis=axes, keepdims=True, dtype=odt)


def _prod_rows(e, dt, rng):
    shape = (e.n_out, e.n_red)
    if dt.kind == "f":
        m = np.full(shape, -1.0, dtype=dt)
        k = min(100, e.n_red // 3)
        if k:
            where = np.argsort(rng.random(shape), axis=1)[:, :2 * k] if e.n_out * e.n_red <= (1 << 22) else \
                np.stack([rng.choice(e.n_red, 2 * k, replace=False) for _ in range(e.n_out)])
            rows = np.arange(e.n_out)[:, None]
            kk = rng.integers(1, k + 1, e.n_out)[:, None]       # 1 .. k twos and as many or fewer halves, per output
            hh = rng.integers(1, k + 1, e.n_out)[:, None]
            idx = np.arange(k)[None, :]
            m[rows, where[:, :k]] = np.where(idx < kk, 2.0, -1.0).astype(dt)
            m[rows, where[:, k:]] = np.where(idx < hh, 0.5, -1.0).astype(dt)
        return m
    info = np.iinfo(dt)
    m = rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True) | dt.type(1)          # odd
    m[(m == 1) | (m == dt.type(-1 if dt.kind == "i" else 1))] = dt.type(3)
    return m


def _prod_ref(v, axes, dt, odt):
    if dt.kind == "f":
        return np.prod(v.astype(np.float64), axis=axes, keepdims=True).astype(odt)     # exact: within 2^+-100
    return np.prod(v, axis=axes, keepdims=True, dtype=odt)


_SPAN = {i8: 200, u8: 190, f16: 2000, i16: 60000, u16: 60000}


def _extreme_rows(e, dt, rng):
    """Per output a permutation of distinct values (as many as the type holds); (rows, lowest - 7, highest + 7)."""
    span = min(e.n_red, _SPAN.get(dt, 1 << 62))
    off = 10 if dt.kind == "u" else -(span // 2)
    vals = np.arange(e.n_red, dtype=np.int64) % span + off
    m = rng.permuted(np.broadcast_to(vals, (e.n_out, e.n_red)), axis=1).astype(dt)
    return m, dt.type(off - 7), dt.type(off + span - 1 + 7)


def _plant(m, pairs, lo, hi):
    m = m.copy()
    for o, (kind, p) in pairs:
        if kind == "hi":
            m[o, p] = hi
        elif kind == "lo":
            m[o, p] = lo
        elif kind == "nan":
            m[o, p] = np.nan
        elif kind == "row":
            m[o, :] = p
    return m


# ---- the checks -----------------------------------------------------------------------------------------------------------------
def _equal(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    np.testing.assert_array_equal(got, ref, err_msg=str(what))      # (NaN equals NaN here; everything else bit for bit)


def _check_entry(e, call, planted, mdopt, on_gpu, dtypes=None):
    opt_values = e.opt[1] if e.opt else (None,)
    if not on_gpu:
        opt_values = opt_values[:1]                                 # (the double has one loop: the option changes nothing)
    for dt in dtypes or e.dtypes:
        ops = e.ops_for(dt)
        arrays = []                                                 # (op, what, device array, reference)

        def case(op, rows, ref_fn, what, salt):
            v = _from_rows(e, rows)
            odt = _out_dtype(op, dt)
            arrays.append((op, what, _upload(e, v, _rng(e, dt, salt)), ref_fn(v, odt), odt))

        if "sum" in ops:
            case("sum", _sum_rows(e, dt, _rng(e, dt, 1)), lambda v, odt: _sum_ref(v, e.axes, dt, odt), "sum", 11)
        if "prod" in ops:
            case("prod", _prod_rows(e, dt, _rng(e, dt, 2)), lambda v, odt: _prod_ref(v, e.axes, dt, odt), "prod", 12)
        if "max" in ops or "min" in ops:
            m, lo, hi = _extreme_rows(e, dt, _rng(e, dt, 3))
            variants = [("permutation", m)]
            if planted:
                items = [(k, p) for p in _positions(e, dt) for k in (("hi", "lo", "nan") if dt.kind == "f" else ("hi", "lo"))]
                if dt.kind == "f":
                    items += [("row", -np.inf), ("row", np.inf)]
                variants += [(f"planted {pairs[:3]} ..", _plant(m, pairs, lo, hi)) for pairs in _groups(e, items)]
            for what, rows in variants:
                v = _from_rows(e, rows)
                d = _upload(e, v, _rng(e, dt, 13))
                for op in ("max", "min"):
                    if op in ops:
                        ref = (np.max if op == "max" else np.min)(v, axis=e.axes, keepdims=True)
                        arrays.append((op, what, d, ref, dt))
        for op in ("any", "all"):
            if op in ops:
                fill = op == "all"
                items = [("lo" if fill else "hi", p) for p in _positions(e, dt)] if planted else []
                rows0 = np.full((e.n_out, e.n_red), fill, dtype=dt)
                variants = [rows0] + [_plant(rows0, pairs, False, True) for pairs in (_groups(e, items) if items else ())]
                for rows in variants:
                    case(op, rows, lambda v, odt, op=op: (np.any if op == "any" else np.all)(v, axis=e.axes, keepdims=True), op, 14)
        for value in opt_values:
            if value is not None:
                mdopt(e.opt[0], value)
            for op, what, d, ref, odt in arrays:
                _equal(call(op, d, e.axes, odt), ref, (e.id, dt.name, op, what, value))
            if "rand" in ops and e.n_red > 1:
                v = (_rng(e, dt, 5).standard_normal(e.shape) * 3 + 10).astype(dt)
                got = call("sum", _upload(e, v, _rng(e, dt, 15)), e.axes, dt)
                wide = v.astype(np.longdouble)
                ref, mass = wide.sum(axis=e.axes, keepdims=True), np.abs(wide).sum(axis=e.axes, keepdims=True)
                u = np.longdouble(2.0) ** (-24 if dt == f32 else -53)
                ratio = float((np.abs(got.astype(np.longdouble) - ref) / (u * mass)).max())
                key = f"{e.reaches} [{e.id}, {dt.name}{'' if value is None else ', ' + e.opt[0] + ' ' + str(value)}]"
                _RATIOS[key] = max(_RATIOS.get(key, 0.0), ratio)
                assert ratio <= min(e.n_red - 1, 34), (e.id, dt.name, ratio)


IDS = [e.id for e in TABLE]


@_twins(IDS)
def _kernel_paths(case, mdopt, on_gpu):
    _check_entry(BY_ID[case], _direct, True, mdopt, on_gpu)


test_kernel_paths, test_kernel_paths_gpu = _kernel_paths


@_twins(IDS)
def _public_functions(case, mdopt, on_gpu):
    """The same entries through nd.sum / nd.prod / nd.max / nd.min / nd.any / nd.all (first dtype, no planted runs)."""
    e = BY_ID[case]
    _check_entry(e, _public, False, mdopt, on_gpu, dtypes=e.dtypes[:1])


test_public_functions, test_public_functions_gpu = _public_functions


# ---- empty extents ----------------------------------------------------------------------------------------------------------------
@_twins(["float32", "int64"])
def _empty_extents(case, mdopt, on_gpu):
    """n_red == 0: sum gives 0 and prod 1 in every output (k_reduce_generic), max has no identity; n_out == 0: nothing to do."""
    dt = np.dtype(case)
    d = nd.asarray(np.zeros((5, 0, 9), dtype=dt))
    _equal(_direct("sum", d, (1,), dt), np.zeros((5, 1, 9), dtype=dt), "sum of nothing")
    _equal(_direct("prod", d, (1,), dt), np.ones((5, 1, 9), dtype=dt), "prod of nothing")
    with pytest.raises(ValueError):
        _direct("max", d, (1,), dt)
    _equal(_direct("sum", d, (0,), dt), np.zeros((1, 0, 9), dtype=dt), "no outputs")
    _equal(_direct("max", nd.asarray(np.zeros((0, 7), dtype=dt)), (1,), dt), np.zeros((0, 1), dtype=dt), "no outputs")


test_empty_extents, test_empty_extents_gpu = _empty_extents


# ---- ticket hygiene ---------------------------------------------------------------------------------------------------------------
TICKETED = [e.id for e in TABLE if e.ticket]


@_twins(["tickets"])
def _tickets_come_back_to_zero(case, mdopt, on_gpu):
    """Every launch form that counts arrivals in the shared ticket block (strips with NB > 1, batched strips, rows with a ticket in
    both forms, k_reduce_all with one and two levels) three times, interleaved with each other: a counter left off zero — or a partial
    row read from another launch — makes the next launch that shares the word merge early or never. Random data (the bits depend on
    the order of summation); every repeat must give the bits of the first."""
    runs = []
    for id_ in TICKETED:
        e = BY_ID[id_]
        for dt in e.dtypes[:2]:
            if dt.kind == "f":
                v = (_rng(e, dt, 6).standard_normal(e.shape) * 3 + 10).astype(dt)
            else:
                v = _from_rows(e, _sum_rows(e, dt, _rng(e, dt, 6)))
            d = _upload(e, v, _rng(e, dt, 16))
            for op in ("sum", "max") if dt == f32 else ("sum",):
                runs.append((e, dt, op, d, _out_dtype(op, dt)))
    assert len(runs) >= 20
    first = [_direct(op, d, e.axes, odt) for e, dt, op, d, odt in runs]
    for order in (range(len(runs) - 1, -1, -1), range(len(runs))):
        for k in order:
            e, dt, op, d, odt = runs[k]
            got = _direct(op, d, e.axes, odt)
            assert got.tobytes() == first[k].tobytes(), (e.id, dt.name, op)


test_tickets_come_back_to_zero, test_tickets_come_back_to_zero_gpu = _tickets_come_back_to_zero


# ---- batches do not leak ----------------------------------------------------------------------------------------------------------
@_twins(["batched-5x200x512", "batched-300x64x256", "batched-3x67x260"])
def _batches_do_not_leak(case, mdopt, on_gpu):
    """The batched strips launch (the leak test of test_middle_axis.py on the plain sums): one element changed changes exactly one
    output of one batch — batches have their own partial rows, ticket words and outputs."""
    e = BY_ID[case]
    outer, n, inner = e.shape
    for dt in e.dtypes:
        h = _from_rows(e, _sum_rows(e, dt, _rng(e, dt, 7)))
        first = _direct("sum", nd.asarray(h), e.axes, dt)
        _equal(first, _sum_ref(h, e.axes, dt, dt), (case, dt.name))
        for b, r, c in ((outer // 2, n // 2, 7), (outer - 1, n - 1, inner - 1), (0, 0, 0)):
            h2 = h.copy()
            h2[b, r, c] += 2
            got = _direct("sum", nd.asarray(h2), e.axes, dt)
            assert np.argwhere(got != first).tolist() == [[b, 0, c]], (case, dt.name, b, r, c)
            assert got[b, 0, c] == first[b, 0, c] + 2
