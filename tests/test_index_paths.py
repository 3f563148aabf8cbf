"""Every launch form of gather, scatter, nonzero and the permutation sort (csrc/index.hip: mdhip_gather, mdhip_scatter,
mdhip_nonzero_*, mdhip_random_permutation) against NumPy, bit for bit.

The centre is TABLE: what an entry reaches (kernel and branch), the base array, the view taken, the key, the value forms, the dtypes,
the option to set. There is no hook that reports which kernel ran: every shape is derived from the launcher's predicates, and the
`reaches` column is confirmed by a kernel trace of the gpu half (profiles/README.md: index_paths_kernel_stats.csv).

Where the numbers come from (V = 16 bytes / element size):
  MD_BLOCK 256, md_grid_for   at most 2048 blocks of 256 threads: 524288 items per grid trip (`addint-elem` has 300 more).
  gather, `runs`              total >= 4096, element size 1 / 4 / 8, last axis contiguous on both sides with length % V == 0, source
                              and output on 16 B, no index along the last axis, every outer stride and index multiplier % V == 0.
                              4095 is the last total below it; every other refusal has an entry of its own at total >= 4096.
  k_gather_runs               units per run lu >= 64 and runs >= 64 (63 units, 63 runs: k_gather_vec). A lane copies units lane + 256 t
                              four at a time while u + 192 < lu, then one at a time: lu 64 / 65 (tail only), 192 / 193 (the last lu
                              with no main trip for lane 0 / the first with one), 255 / 256 / 257, 320, 511 / 512 (two main trips
                              begin at 449), 777. 1024 blocks x 4 waves = 4096 runs per trip: 4097 runs give one wave a second trip.
  scatter, serial             total <= 128 (k_scatter_serial); 129 is the first total on the sorted paths.
  run_geometry                last plan axis contiguous, >= 8 long, no index along it, rows identical or disjoint: the sort is at ROW
                              granularity (k_run_offsets, k_run_apply / k_run_apply_vec); everything else is element-granular
                              (k_elem_offsets, k_elem_apply, k_elem_apply_long).
  k_run_apply_vec, ADD        contributions four at a time, then a tail: multiplicities 1, 2, 3, 4, 5, 7, 8, 9 and 200 in one plan.
  run_vectorisable            V >= 2, L % V == 0, destination on 16 B, outer strides and index multipliers % V == 0, value
                              contiguous along the last axis, on 16 B, its outer strides % V == 0: one entry per refusal.
  census                      total > 4096 and at most 2^22 row keys: k_check_bounds_dups; unique rows skip the sort.
  RS_TILE 2048                the sort's tile: P 2048 / 2049; 256 counters per tile, scanned 2048 at a time: a second chunk from
                              P > 16384 (16385), a second round of k_rs_scan_totals from 256 chunks, P > 4194304 (gpu only). Eight
                              key bits per pass: 2^22 + 1 row keys are 23 bits, three passes (the result is in the second half);
                              a destination of 2^24 + 5 elements is 25 bits, four passes; the permutation sorts 64 bits, eight.
  ELEM_SHORT 64               up to 64 contributions a lane adds itself; 65 and more go to a wave (k_elem_apply_long), 64 at a time,
                              which ends on a chunk with fewer than 64: counts 63 .. 66, 127 .. 129, 192, 1000; a long destination
                              that ends exactly at `total`; 4100 long destinations for the 4096 waves launched.
  NZ_CHUNK 2048               elements per block of nonzero, 8 per thread; k_nz_scan gives each of 256 lanes ceil(nb / 256) blocks:
                              nb 256 (n = 256 * 2048) and 257 (one more element) is where idle lanes first appear.

Data — every comparison is on raw bits (the arrays viewed as unsigned integers of the element size; NaN payloads and -0.0 count),
there is no tolerance anywhere:
  gather, SET   every element distinct: an element counter times an odd constant, reinterpreted in the dtype (1- and 2-byte types:
                the counter mod 2^bits with a row-dependent offset; bool: a row-dependent 0 / 1 pattern).
  ADD, floats   standard normals * 10^uniform(-3, 3) (float16: a narrower spread, so that no sum overflows): the order of the
                additions changes bits — the CPU twin asserts that the reversed plan order gives other bits wherever a plan has
                duplicates and a value that varies from one plan row to the next (dense, the strided view, (P, 1)). float16: np.add.at on a float16 array (rounds after every contribution).
  ADD, integers full-range values (wrap-around); bool: logical or.
  indices       int64, and int32 for the first dtype of every entry; negative ones mixed in, exactly -extent among them.
  padding       destinations, sources and gather outputs are views inside a larger base that holds a sentinel (NaN for floats, a fixed
                pattern for integers): the whole base is compared. A gather writes into a block of this module's own, pre-filled with
                the sentinel (nd._build_plan + lib.gather, as nd.getitem does at its end).

Each test has a twin: unmarked on the CPU double (skipped when a GPU is bound) — it proves that data and references are right — and
gpu-marked on the product library. Three entries are gpu-only, for their size or their NumPy time: census-over-2^22,
sorted-totals-second-round and runs-vec-L16B*256-P16385 (float32 only; the other row lengths carry P = 16385 on both twins).

Exempt from the order-sensitivity check: the row-invariant (1, L) and scalar value forms — every contribution to a destination is
the same number there, so no order of adding them can differ; the dense entry of the same plan carries the check. Every boundary
of 2048 elements gets its single non-zero in bool only (test_nonzero_every_boundary at 257 blocks, and gpu-only at 3 * 2^19 + 5);
the other dtypes take the first two, the middle and the last two boundaries of every size."""
import ctypes as C
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

from minidiff_amd import ndarray as nd

f16, f32, f64 = np.dtype(np.float16), np.dtype(np.float32), np.dtype(np.float64)
i8, i16, i32, i64 = np.dtype(np.int8), np.dtype(np.int16), np.dtype(np.int32), np.dtype(np.int64)
u8, u16, u32, u64 = np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.uint32), np.dtype(np.uint64)
b8 = np.dtype(np.bool_)
ALL12 = (b8, i32, i64, f32, f64, u32, u64, i8, u8, i16, u16, f16)
SMALL = (i8, u8, i16, u16, f16)
BY_SIZE = {1: (i8, b8), 2: (f16, i16), 4: (f32, i32), 8: (f64, i64)}
S = slice
PAD = 16                                    # elements around a gather's output block (a multiple of 16 B for every size)
MULTS = (1, 2, 3, 4, 5, 7, 8, 9, 200)       # contributions per destination row, k_run_apply_vec's unroll by four and its tail
COUNTS = (1000, 1, 2, 63, 64, 66, 127, 128, 129, 192, 65)   # contributions per destination, ELEM_SHORT and the 64-position chunks
GRID_TRIP = 2048 * 256                      # md_grid_for: at most 2048 blocks of MD_BLOCK threads


class Entry:
    def __init__(self, kind, id, reaches, base, key, dtypes, view=None, forms=("dense",), modes=("set", "add"), add_dtypes=None, opt=None,
                 opt_only=False, gpu_only=False, along=None, seed=2):
        self.kind, self.id, self.reaches, self.base, self.key, self.dtypes = kind, id, reaches, base, key, tuple(dtypes)
        self.view, self.forms, self.modes, self.add_dtypes = view, forms, modes, add_dtypes
        self.opt, self.opt_only, self.gpu_only, self.along, self.seed = opt, opt_only, gpu_only, along, seed

    def base_shape(self, dt):
        return self.base(16 // dt.itemsize) if callable(self.base) else tuple(self.base)

    def cut(self, a):
        return a if self.view is None else self.view(a)


TABLE = []


def _g(id, reaches, base, key, sizes, **k):
    TABLE.append(Entry("gather", id, reaches, base, key, [BY_SIZE[s][0] for s in sizes] + [BY_SIZE[s][1] for s in sizes[:1]], **k))


def _s(id, reaches, base, key, dtypes, **k):
    TABLE.append(Entry("scatter", id, reaches, base, key, dtypes, **k))


def _indices(rng, extent, shape):
    """Valid indices of either sign with duplicates; the first is exactly -extent, the second its non-negative alias (a duplicate
    destination whatever else is drawn), the last is extent - 1."""
    ix = rng.integers(-extent, extent, shape)
    ix.flat[0] = -extent
    if ix.size > 2:
        ix.flat[1] = 0
    if ix.size > 1:
        ix.flat[-1] = extent - 1
    return ix


def _mixed_sign(rng, ix, extent):
    return np.where(rng.random(ix.shape) < 0.3, ix - extent, ix)


def rows(n):
    """a[idx]: an index array of shape n over the first axis."""
    return lambda rng, shape: (_indices(rng, shape[0], n),)


def rows_then(n, sl):
    return lambda rng, shape: (_indices(rng, shape[0], n), sl)


def on_axis1(n):
    return lambda rng, shape: (S(None), _indices(rng, shape[1], n))


def mult_rows(P):
    """P plan rows over the first axis: destination rows 0 .. 8 get exactly MULTS contributions, the others share the rest."""
    def key(rng, shape):
        special = np.repeat(np.arange(len(MULTS)), MULTS)
        rest = rng.integers(len(MULTS), shape[0], P - special.size)
        return (_mixed_sign(rng, rng.permutation(np.concatenate([special, rest])), shape[0]),)
    return key


def counted(counts):
    """An element plan over a 1-D destination: destination 3 * j gets exactly counts[j] contributions, in shuffled plan order."""
    def key(rng, shape):
        assert shape[0] > 3 * (len(counts) - 1)
        return (_mixed_sign(rng, rng.permutation(np.repeat(3 * np.arange(len(counts)), counts)), shape[0]),)
    return key


def permutation(dup):
    def key(rng, shape):
        ix = _mixed_sign(rng, rng.permutation(shape[0]), shape[0])
        if dup:
            ix[-1] = ix[0]              # the first and the last plan row aim at one destination
        return (ix,)
    return key


# ---- gather (mdhip_gather) -------------------------------------------------------------------------------------------------------
R = 37                                   # source rows: fewer than plan rows, so every plan repeats rows
_g("gather-4095", "k_gather: total 4095, below the vector threshold", (R, 63), rows(65), (1, 2, 4, 8))
_g("gather-last-axis", "k_gather: an index on the last axis (a[:, idx])", (70, 100), on_axis1(64), (1, 2, 4, 8))
_g("gather-col-off16", "k_gather: a column slice off 16 B (a[idx, 3:], rows of 64 in a pitch of 72)", (R, 72), rows_then(64, S(3, None)), (4, 8),
   view=lambda a: a[:, :67])
_g("gather-len-mod-V", "k_gather: row length 65, % V != 0", (R, 80), rows(64), (1, 4, 8), view=lambda a: a[:, :65])
_g("gather-size-2", "k_gather: element size 2, whole rows", (R, 64), rows(64), (2,))
_g("gather-stride-mod-V", "k_gather: row stride 258, % V != 0", (R, 258), rows(16), (4, 1), view=lambda a: a[:, :256])
_g("gather-src-off16", "k_gather: the source's first element off 16 B", (R * 64 + 8,), rows(64), (4, 8, 1),
   view=lambda a: a[1:1 + R * 64].reshape(R, 64))
_g("vec-63-units", "k_gather_vec: 63 units per run", lambda V: (R, 63 * V), rows(64), (4, 1, 8))
_g("vec-63-runs", "k_gather_vec: 63 runs of 1024 elements", (R, 1024), rows(63), (4, 1, 8))
RUNS = ("gather_runs", 0)
for lu in (64, 65, 192, 193, 255, 256, 257, 320, 511, 512, 777):
    _g(f"runs-lu{lu}", f"k_gather_runs: {lu} units per run, 64 runs; gather_runs = 0: k_gather_vec", lambda V, lu=lu: (R, lu * V), rows(64),
       (4, 1, 8) if lu in (65, 257, 777) else (4,), opt=RUNS)
_g("runs-second-trip", "k_gather_runs: 4097 runs of 65 units, a second trip of wave 0", lambda V: (R, 65 * V), rows(4097), (4,), opt=RUNS)
_g("runs-2d-index", "k_gather_runs: a 2-D index array", lambda V: (R, 65 * V), rows((8, 8)), (4, 8), opt=RUNS)
_g("runs-middle-axis", "k_gather_runs: an index on a middle axis (t[:, i3]), runs = 4 x 16", lambda V: (4, R, 65 * V), on_axis1(16), (4, 1), opt=RUNS)
_g("runs-along-axis", "k_gather_runs: take_along_axis(arr, idx of shape (64, 1), 0)", lambda V: (R, 65 * V), None, (4, 8), opt=RUNS, along=(64, 0))
_g("runs-flipped", "k_gather_runs: a flipped source (a[::-1][idx]), negative index multiplier", lambda V: (R, 65 * V), rows(64), (4, 1), opt=RUNS,
   view=lambda a: a[::-1])
_g("runs-col-offset", "k_gather_runs: an aligned column offset (a[idx, V:]; float32: a[idx, 4:])", lambda V: (R, 66 * V),
   lambda rng, shape: (_indices(rng, shape[0], 64), S(shape[1] // 66, None)), (4, 8), opt=RUNS)

# ---- scatter (mdhip_scatter) -----------------------------------------------------------------------------------------------------
D = 64                                   # destination rows of the row plans
F, WIDE_SET = (f32, f64), (f32, f64, i32, i64, b8)
pad_rows = lambda a: a[1:-1]             # noqa: E731   (a sentinel row before and after; the view stays on 16 B when the rows are)
for total in (1, 128):
    _s(f"serial-{total}", f"k_scatter_serial: total {total}", (56,), rows(total), ALL12, view=lambda a: a[3:53], forms=("dense", "scalar"))
_s("serial-next-129", "total 129, the data shape of serial-128: k_elem_apply (integer ADD: k_scatter_add_int)", (56,), rows(129), ALL12,
   view=lambda a: a[3:53], forms=("dense", "scalar"))

for L in (8, 64, "16B*256"):
    for P in ("min", 2048, 2049, 16385):
        def base(V, L=L):
            return (D + 2, 256 * V if L == "16B*256" else L)
        if P == "min":                   # the fewest rows with total > 128
            key = lambda rng, shape: (_indices(rng, shape[0], -(-129 // shape[1])),)      # noqa: E731
        else:
            key = mult_rows(P)
        big = L == "16B*256" and P == 16385      # (64 MiB of values, seconds of np.add.at: gpu only, float32 only)
        _s(f"runs-vec-L{L}-P{P}", f"scatter_runs + k_run_apply_vec (bool at L 8: k_run_apply): rows of {L}, {P} plan rows", base, key,
           (f32,) if big else WIDE_SET if L != "16B*256" else F, view=pad_rows, add_dtypes=F, forms=("dense", "row", "scalar") if P == 2049 else ("dense",),
           gpu_only=big)

_s("apply-len-mod-V", "k_run_apply: L = 10, % V != 0", (D + 2, 10), mult_rows(300), (f32, i32), view=pad_rows, add_dtypes=(f32,))
_s("apply-dst-off16", "k_run_apply: destination off 16 B", (D * 64 + 8,), mult_rows(300), F, view=lambda a: a[1:1 + D * 64].reshape(D, 64))
_s("apply-dst-stride", "k_run_apply: destination row stride 66, % V != 0", (D, 66), mult_rows(300), (f32, i32), view=lambda a: a[:, :64], add_dtypes=(f32,))
_s("apply-val-col", "k_run_apply: value broadcast along the last axis, (P, 1)", (D + 2, 64), mult_rows(300), F, view=pad_rows, forms=("col",))
_s("apply-val-view", "k_run_apply: value a [:, 1:65] view of (P, 66): off 16 B, row stride % V != 0", (D + 2, 64), mult_rows(300), F, view=pad_rows,
   forms=("vview",))
_s("apply-small", "k_run_apply: 1- and 2-byte types never vectorise", (D + 2, 64), mult_rows(300), SMALL, view=pad_rows, forms=("dense", "scalar"))
_s("geom-flipped", "scatter_runs: a flipped destination (d[::-1]), negative index multiplier", (D, 64), mult_rows(300), F, view=lambda a: a[::-1])
_s("geom-middle-axis", "scatter_runs: an index on a middle axis, unit = the row", (3, D, 16), on_axis1(100), F)
_s("geom-short-run", "scatter_runs + k_run_apply: a run shorter than the row (d[:, 5:42])", (D, 48), mult_rows(300), F, view=lambda a: a[:, 5:42])
_s("geom-two-outer", "scatter_runs: two outer plan axes longer than 1 (a 2-D index array)", (D, 16), rows((10, 30)), F)

CENSUS = ("scatter_census", 0)
_s("census-unique", "k_check_bounds_dups: unique rows, the sort is skipped; scatter_census = 0: k_check_bounds + the sort", (602, 8), permutation(False),
   F, view=pad_rows, opt=CENSUS)
_s("census-one-dup", "k_check_bounds_dups: first and last plan row aim at one destination, the sort runs; scatter_census = 0: the same bits",
   (602, 8), permutation(True), F, view=pad_rows, opt=CENSUS, seed=3)     # (seed: two contributions whose order shows, in both types)
_s("census-over-2^22", "2^22 + 1 row keys: no census, k_check_bounds + a three-pass sort (the sorted half is 1)", ((1 << 22) + 3, 8),
   lambda rng, shape: (np.concatenate([_indices(rng, shape[0], 2500), rng.integers(0, 300, 2500)]),), (f32,), view=pad_rows, gpu_only=True)

INTS = (i32, i64, u32, u64)
_s("addint-run", "k_scatter_add_int: a run plan, heavy duplicates", (D + 2, 16), lambda rng, shape: (_indices(rng, 5, 3000),), INTS, view=pad_rows,
   modes=("add",), forms=("dense", "scalar"))
_s("addint-elem", "k_scatter_add_int: an element plan of one grid trip + 300", (1006,), rows(GRID_TRIP + 300), INTS, view=lambda a: a[3:-3],
   modes=("add",), forms=("dense", "scalar"))

SORTED = ("scatter_sorted", 0)
_SORTED_SMALL = [
    ("counts-long-first", "destinations of 1 .. 1000 contributions, the 1000 first in sorted order, a 65 last: a long destination ends at total",
     (40,), counted(COUNTS), ALL12, {"view": lambda a: a[3:-3], "forms": ("dense", "scalar")}),
    ("counts-long-last", "the same counts reversed: a 65 first, the 1000 last", (40,), counted(COUNTS[::-1]), ALL12,
     {"view": lambda a: a[3:-3], "forms": ("dense", "scalar")}),
    ("total-129", "an index on the last axis, total 3 x 43 = 129", (3, 50), on_axis1(43), ALL12, {}),
    ("total-2048", "an index on the last axis, total 4 x 512 = 2048: one sort tile", (4, 50), on_axis1(512), ALL12, {}),
    ("total-2049", "an index on the last axis, total 3 x 683 = 2049: two sort tiles", (3, 50), on_axis1(683), ALL12, {}),
]
for id_, what, base_, key_, dts_, kw_ in _SORTED_SMALL:
    _s("sorted-" + id_, "scatter_sorted (k_elem_offsets, the sort, k_elem_apply, k_elem_apply_long): " + what, base_, key_, dts_, **kw_)
    _s("ordered-" + id_, "scatter_ordered by scatter_sorted = 0 (k_offsets, rounds of k_bid + k_apply): " + what, base_, key_, dts_, opt=SORTED, opt_only=True,
       **kw_)
_s("sorted-short-rows", "scatter_sorted: whole rows of L = 4 < 8 are an element plan", (D, 4), rows(500), F + (i8,))
_s("sorted-4100-long", "k_elem_apply_long: 4100 destinations of 65 contributions, more than the 4096 waves", (4100,),
   lambda rng, shape: (_mixed_sign(rng, rng.permutation(np.repeat(np.arange(4100), 65)), 4100),), (f32,))
_s("sorted-two-indices", "scatter_sorted: two index arrays into a strided, flipped destination (d[::-1, ::2]), scalar value", (40, 60),
   lambda rng, shape: (_indices(rng, shape[0], 500), _indices(rng, shape[1], 500)), (f32, i8), view=lambda a: a[::-1, ::2], forms=("scalar",))
_s("sorted-span-2^24", "scatter_sorted: a destination of 2^24 + 5 elements, 25 key bits, four passes", ((1 << 24) + 5 + 6,), rows(300), (i8,),
   view=lambda a: a[3:-3])
_s("sorted-totals-second-round", "scatter_sorted: 4194304 + 2049 positions into 1000 bins: 257 chunks, a second round of k_rs_scan_totals", (1006,),
   rows(4194304 + 2049), (f32,), view=lambda a: a[3:-3], modes=("add",), gpu_only=True)

BY_ID = {e.id: e for e in TABLE}
assert len(BY_ID) == len(TABLE)


# ---- plumbing --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def eager():
    prev = nd.set_lazy(False)
    yield
    nd.set_lazy(prev)


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


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.dtype(f"u{a.dtype.itemsize}"))


def _same_bits(got, ref, what):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    g, r = _bits(got), _bits(ref)
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        raise AssertionError(f"{what}: {len(bad)} of {g.size} elements differ, first at {bad[0].tolist()}: got {g[tuple(bad[0])]:#x}, expected {r[tuple(bad[0])]:#x}")


def _sentinel(dt):
    if dt.kind == "f":
        return dt.type(np.nan)
    if dt == b8:
        return np.True_
    return np.array([0x5A5A5A5A5A5A5A5A & ((1 << (8 * dt.itemsize - 1)) - 1)]).astype(dt)[0]


def _payload(shape, dt, salt=0):
    """Distinct elements: a counter times an odd constant in the dtype's own bits (wide types); the counter mod 2^bits with a
    row-dependent offset (1- and 2-byte types)."""
    n = int(np.prod(shape, dtype=np.int64))
    if dt.itemsize >= 4:
        u = np.dtype(f"u{dt.itemsize}")
        mul = u.type(0x9E3779B1 if dt.itemsize == 4 else 0x9E3779B97F4A7C15)
        with np.errstate(over="ignore"):
            c = (np.arange(n, dtype=u) + u.type(salt + 1)) * mul
        return c.view(dt).reshape(shape)
    L = shape[-1]
    col, row = np.arange(L, dtype=np.int64)[None, :], np.arange(n // L, dtype=np.int64)[:, None]
    if dt == b8:
        return ((((col + row) ^ (col >> 3) ^ (row >> 2)) + salt) & 1).astype(b8).reshape(shape)
    u = np.dtype(f"u{dt.itemsize}")
    return ((col + 37 * row + salt) % (1 << (8 * dt.itemsize))).astype(u).view(dt).reshape(shape)


def _check_distinct(a, what):
    """The self-check of _payload (CPU twin): every element distinct; for the narrow types every window of 2^bits elements of a row,
    and neighbouring rows from one another."""
    dt, bits = a.dtype, _bits(a)
    if dt.itemsize >= 4:
        assert np.unique(bits).size == bits.size, what
    elif dt != b8:
        rows_ = bits.reshape(-1, bits.shape[-1])
        w = min(rows_.shape[1], 1 << (8 * dt.itemsize))
        assert all(np.unique(r[:w]).size == w for r in rows_[:: max(1, len(rows_) // 8)]), what
        assert len(rows_) < 2 or (rows_[1:, 0] != rows_[:-1, 0]).all(), what


def _noise(rng, shape, dt):
    """ADD operands: floats over several decades (the order of additions changes bits), integers over the full range, bools."""
    if dt.kind == "f":
        lo, hi = (-3, 3) if dt != f16 else (-2, 1)
        return (rng.standard_normal(shape) * 10.0 ** rng.uniform(lo, hi, shape)).astype(dt)
    if dt == b8:
        return rng.random(shape) < 0.2
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)


def _in_base(e, dt, fill):
    """The base array (all sentinel) with fill(shape of the view) inside the view."""
    base = np.full(e.base_shape(dt), _sentinel(dt), dtype=dt)
    v = e.cut(base)
    assert np.shares_memory(v, base)
    v[...] = fill(v.shape)
    return base


def _device_key(key, idt):
    return tuple(nd.asarray(k.astype(idt)) if isinstance(k, np.ndarray) else k for k in key)


def _with_option(e, mdopt, on_gpu):
    """The option values an entry runs under: None (the default, put in place explicitly), then the entry's own; the default is back
    when the generator ends. The double has one loop per entry point: there the option changes nothing and the default alone runs
    (an opt_only entry: once, as it is)."""
    if not (e.opt and on_gpu):
        yield None
        return
    default = C.c_int64()
    nd._lib().debug_get_option(e.opt[0].encode(), C.byref(default))
    try:
        for value in ([] if e.opt_only else [None]) + [e.opt[1]]:
            mdopt(e.opt[0], default.value if value is None else value)
            yield value
    finally:
        mdopt(e.opt[0], default.value)     # (the callers loop over dtypes, modes and forms: every default run starts from the default)


# ---- gather ----------------------------------------------------------------------------------------------------------------------
def _gather_into_own_block(a, key, along):
    """a[key] (or take_along_axis) through the C-ABI into a sentinel-filled block of this module's own -> (whole block, out shape)."""
    if along is None:
        entries, has_adv = nd._parse_key(a, key)
        assert has_adv
        plan, oshape, ptr, keep = nd._build_plan(a, entries)
    else:
        plan, oshape, keep = nd._along_axis_plan(a, key[0], along)
        ptr = a.ptr
    n = int(np.prod(oshape, dtype=np.int64))
    block = nd.asarray(np.full(n + 2 * PAD, _sentinel(a.dtype), dtype=a.dtype))
    out = block[PAD:PAD + n].reshape(oshape)
    assert out.ptr - block.ptr == PAD * a.dtype.itemsize            # (a view of the block, on 16 B when the block is)
    nd._lib().gather(plan, ptr, a._code, out.desc())
    del keep
    return block.get(), oshape


def _gather_case(e, dt, rng):
    base = _in_base(e, dt, lambda shape: _payload(shape, dt))
    src = e.cut(base)
    if e.along is None:
        key = e.key(rng, src.shape)
        ref = src[key]
    else:
        key = (_indices(rng, src.shape[e.along[1]], (e.along[0], 1)),)
        ref = np.take_along_axis(src, key[0], e.along[1])
    return base, src, key, ref


def _check_gather(e, mdopt, on_gpu):
    for k, dt in enumerate(e.dtypes):
        for idt in (i64, i32) if k == 0 else (i64,):
            base, src, key, ref = _gather_case(e, dt, _rng(e, dt, 1))
            if not on_gpu:
                _check_distinct(src, (e.id, dt.name))
            dsrc = e.cut(nd.asarray(base))
            dkey = _device_key(key, idt)
            expect = np.full(ref.size + 2 * PAD, _sentinel(dt), dtype=dt)
            expect[PAD:PAD + ref.size] = ref.ravel()
            seen = []
            for value in _with_option(e, mdopt, on_gpu):
                got, oshape = _gather_into_own_block(dsrc, dkey, None if e.along is None else e.along[1])
                assert oshape == ref.shape, (e.id, oshape, ref.shape)
                _same_bits(got, expect, (e.id, dt.name, idt.name, value))
                seen.append(got.tobytes())
            assert len(set(seen)) == 1
            if e.along is None:         # the public route (the allocator's block instead of this module's)
                _same_bits(dsrc[dkey].get(), ref, (e.id, dt.name, idt.name, "getitem"))
            else:
                _same_bits(nd.take_along_axis(dsrc, dkey[0], e.along[1]).get(), ref, (e.id, dt.name, idt.name, "take_along_axis"))


# ---- scatter ---------------------------------------------------------------------------------------------------------------------
def _value(form, oshape, dt, mode, rng):
    """-> (NumPy operand, function giving the device operand)."""
    make = (lambda shape: _payload(shape, dt, salt=7)) if mode == "set" else (lambda shape: _noise(rng, shape, dt))
    lead, L = tuple(oshape[:-1]), oshape[-1]
    if form == "scalar":
        s = make((1, 8)).ravel()[5]
        return s, lambda: s
    if form == "vview":                 # a [:, 1:L + 1] view of rows of L + 2
        wide = np.full(lead + (L + 2,), _sentinel(dt), dtype=dt)
        wide[..., 1:L + 1] = make(oshape)
        return wide[..., 1:L + 1], lambda: nd.asarray(wide)[..., 1:L + 1]
    shape = {"dense": tuple(oshape), "row": (1,) * len(lead) + (L,), "col": lead + (1,)}[form]
    v = make(shape)
    return v, lambda: nd.asarray(v)


def _numpy_scatter(view, key, val, mode):
    if mode == "set":
        view[key] = val
    else:
        with np.errstate(all="ignore"):
            np.add.at(view, key, val)


def _device_scatter(view, key, val, mode):
    if mode == "set":
        view[key] = val
    else:
        nd.index_add(view, key, val)


def _check_order_matters(e, dt, base, key, val, ref_view):
    """A condition on the DATA of a float ADD (CPU twin): where the plan has duplicate destinations and the value is dense, adding
    the same contributions in reversed plan order gives other bits in at least one destination."""
    start = np.ascontiguousarray(e.cut(base))
    offs = np.arange(start.size).reshape(start.shape)[key].ravel()
    vals = np.broadcast_to(val, np.arange(start.size).reshape(start.shape)[key].shape).ravel()
    fwd, rev = start.ravel().copy(), start.ravel().copy()
    with np.errstate(all="ignore"):
        np.add.at(fwd, offs, vals)
        np.add.at(rev, offs[::-1], vals[::-1])
    assert np.array_equal(_bits(fwd), _bits(ref_view).ravel()), (e.id, dt.name, "flat model of the plan")
    if np.unique(offs).size < offs.size:
        assert not np.array_equal(_bits(fwd), _bits(rev)), (e.id, dt.name, "the reversed order gives the same bits: choose other data")


def _scatter_modes(e, dt):
    for mode in e.modes:
        if mode == "add" and e.add_dtypes is not None and dt not in e.add_dtypes:
            continue
        yield mode


def _check_scatter(e, mdopt, on_gpu):
    for k, dt in enumerate(e.dtypes):
        for idt in (i64, i32) if k == 0 else (i64,):
            for mode in _scatter_modes(e, dt):
                for form in e.forms:
                    rng = _rng(e, dt, e.seed)
                    base = _in_base(e, dt, lambda shape: _payload(shape, dt) if mode == "set" else _noise(rng, shape, dt))
                    key = e.key(rng, e.cut(base).shape)
                    oshape = np.empty(e.cut(base).shape, dtype=np.bool_)[key].shape
                    val, dval = _value(form, oshape, dt, mode, rng)
                    ref = base.copy()
                    _numpy_scatter(e.cut(ref), key, val, mode)
                    if not on_gpu and idt == i64:
                        if mode == "set" and form in ("dense", "vview"):
                            _check_distinct(np.ascontiguousarray(val), (e.id, dt.name, form))
                        if mode == "add" and dt.kind == "f" and form in ("dense", "vview", "col"):
                            _check_order_matters(e, dt, base, key, val, e.cut(ref))
                    dkey = _device_key(key, idt)
                    for value in _with_option(e, mdopt, on_gpu):
                        dbase = nd.asarray(base)
                        _device_scatter(e.cut(dbase), dkey, dval(), mode)
                        _same_bits(dbase.get(), ref, (e.id, dt.name, idt.name, mode, form, value))


def _check_entry(case, mdopt, on_gpu):
    e = BY_ID[case]
    (_check_gather if e.kind == "gather" else _check_scatter)(e, mdopt, on_gpu)


test_paths, test_paths_gpu = _twins([e.id for e in TABLE if not e.gpu_only])(_check_entry)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [e.id for e in TABLE if e.gpu_only])
def test_large_paths_gpu(lib, on_gpu, mdopt, case):
    """The entries whose arrays are too large for the CPU twin (the census bound of 2^22 row keys: a 128 MiB destination; 4.2 M
    positions): the references are NumPy's all the same."""
    assert on_gpu and lib.target == "hip:gfx950"
    _check_entry(case, mdopt, True)


# ---- out of range ----------------------------------------------------------------------------------------------------------------
# (kernel, source shape, plan rows, places of the bad index: the first run, the last run, and for k_gather_runs a run of the second trip)
GATHER_OOB = {
    "k_gather": ((20, 63), 65, (0, 64)),
    "k_gather_vec": ((20, 252), 64, (0, 63)),
    "k_gather_runs": ((20, 260), 4100, (0, 4099, 4097)),
}


@_twins(sorted(GATHER_OOB))
def _gather_out_of_range(case, mdopt, on_gpu):
    """One bad index (extent, -extent - 1) among valid ones: IndexError from each of the three kernels (k_gather_runs sets the flag
    from lane 0 of the wave that owns the run)."""
    shape, n, places = GATHER_OOB[case]
    src = nd.asarray(_payload(shape, f32))
    rng = np.random.default_rng(5)
    for place in places:
        for bad in (shape[0], -shape[0] - 1):
            ix = _indices(rng, shape[0], n)
            ix[place] = bad
            with pytest.raises(IndexError):
                _gather_into_own_block(src, (nd.asarray(ix),), None)
    ix = _indices(rng, shape[0], n)
    _same_bits(_gather_into_own_block(src, (nd.asarray(ix),), None)[0][PAD:-PAD].reshape(n, shape[1]), src.get()[ix], case)   # (and none: no error sticks)


test_gather_out_of_range, test_gather_out_of_range_gpu = _gather_out_of_range

# (bounds kernel, destination shape, plan rows): an element plan; a run plan of total <= 4096; a run plan of total > 4096
SCATTER_OOB = {
    "k_check_bounds, step 1": ((50,), 200),
    "k_check_bounds, runs": ((64, 16), 100),
    "k_check_bounds_dups": ((64, 16), 300),
}


@_twins(sorted(SCATTER_OOB))
def _scatter_out_of_range(case, mdopt, on_gpu):
    """One bad index in the LAST position: IndexError, and nothing is written — the destination keeps its bits."""
    shape, n = SCATTER_OOB[case]
    rng = np.random.default_rng(6)
    before = _noise(rng, shape, f32)
    val = nd.asarray(_noise(rng, (n,) + shape[1:], f32))
    for bad in (shape[0], -shape[0] - 1):
        for mode in ("set", "add"):
            ix = _indices(rng, shape[0], n)
            ix[-1] = bad
            d = nd.asarray(before)
            with pytest.raises(IndexError):
                _device_scatter(d, (nd.asarray(ix),), val, mode)
            _same_bits(d.get(), before, (case, bad, mode))


test_scatter_out_of_range, test_scatter_out_of_range_gpu = _scatter_out_of_range


# ---- nonzero ---------------------------------------------------------------------------------------------------------------------
NZ_SIZES = (1, 7, 8, 9, 2047, 2048, 2049, 256 * 2048, 256 * 2048 + 1, 3 * 524288 + 5)
NZ_SHAPES = ((3, 683), (257, 2049), (8, 16, 4097), (2, 1, 5))         # 2049 and 524416 / 526593 elements: 2 and 257 / 258 blocks


def _nz_values(rng, n, dt, density):
    """Zeros and non-zeros; floats: +0.0 and -0.0 are zero, NaN, a denormal, inf and ordinary numbers are not."""
    hit = rng.random(n) < density
    if dt.kind == "f":
        nz = np.array([np.nan, np.finfo(dt).smallest_subnormal, -np.finfo(dt).smallest_subnormal, np.inf, -np.inf, 1.5, -2.0], dtype=dt)
        return np.where(hit, nz[rng.integers(0, len(nz), n)], np.array([0.0, -0.0], dtype=dt)[rng.integers(0, 2, n)]).astype(dt)
    if dt == b8:
        return hit
    return np.where(hit, np.array([1, -1, np.iinfo(dt).min, 256, 1 << 24], dtype=dt)[rng.integers(0, 5, n)], 0).astype(dt)


def _nz_single_positions(n, every_chunk):
    p = {0, n - 1, 7, 8, 2047 - 8, 2048 + 7, 2048 + 8}                  # the ends; the 8-element per-thread boundary inside a chunk
    chunks = list(range(2048, n, 2048))
    some = chunks[:2] + chunks[len(chunks) // 2:len(chunks) // 2 + 1] + chunks[-2:]
    for c in chunks if every_chunk else some:
        p |= {c - 1, c}                                                 # both sides of a 2048-element boundary
    for c in some:
        p |= {c + 7, c + 8}
    return sorted(q for q in p if 0 <= q < n)


@_twins(["bool", "int32", "int64", "float32", "float64"])
def _nonzero(case, mdopt, on_gpu):
    """k_nz_count, k_nz_scan, k_nz_fill: all zero, all non-zero, random half, and ONE non-zero at the ends and on both sides of the
    chunk and thread boundaries (the first two, the middle and the last two chunk boundaries; every one: the next test)."""
    dt = np.dtype(case)
    rng = np.random.default_rng([11, dt.num])
    for n in NZ_SIZES:
        for density in (0.0, 1.0, 0.5):
            x = _nz_values(rng, n, dt, density)
            ref = np.flatnonzero(x)
            assert ref.size == (0 if density == 0.0 else n if density == 1.0 else ref.size)
            got = nd.flatnonzero(nd.asarray(x)).get()
            assert got.dtype == np.int64 and np.array_equal(got, ref), (case, n, density)
        d = nd.asarray(np.zeros(n, dtype=dt))
        one = _nz_values(rng, 1, dt, 1.0)[0]
        for p in _nz_single_positions(n, every_chunk=False):
            d[p] = one
            assert nd.flatnonzero(d).get().tolist() == [p], (case, n, p)
            d[p] = dt.type(0)
    for shape in NZ_SHAPES:
        x = _nz_values(rng, int(np.prod(shape)), dt, 0.5).reshape(shape)
        dx = nd.asarray(x)
        for got, ref in zip(nd.nonzero(dx), np.nonzero(x)):
            assert np.array_equal(got.get(), ref), (case, shape)
        assert np.array_equal(nd.argwhere(dx).get(), np.argwhere(x)), (case, shape)


test_nonzero, test_nonzero_gpu = _nonzero


def _every_boundary(n):
    """One non-zero on each side of EVERY 2048-element boundary (bool): each block's offset and each lane's share of k_nz_scan is met
    by a position of its own."""
    d = nd.asarray(np.zeros(n, dtype=b8))
    for p in _nz_single_positions(n, every_chunk=True):
        d[p] = True
        assert nd.flatnonzero(d).get().tolist() == [p], (n, p)
        d[p] = False


@_twins([256 * 2048 + 1])
def _nonzero_every_boundary(case, mdopt, on_gpu):
    """257 blocks: k_nz_scan's lanes 0 .. 128 take two blocks each (the last of them one), the others none."""
    _every_boundary(case)


test_nonzero_every_boundary, test_nonzero_every_boundary_gpu = _nonzero_every_boundary


@pytest.mark.gpu
def test_nonzero_every_boundary_largest_gpu(lib, on_gpu):
    """3 * 2^19 + 5 elements, 769 blocks, four per lane: 1538 boundary positions (gpu only: the double takes 7 ms per position)."""
    assert on_gpu and lib.target == "hip:gfx950"
    _every_boundary(3 * 524288 + 5)


# ---- permutation: the 64-bit, eight-pass use of the sort ---------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _perm_golden():
    spec = importlib.util.spec_from_file_location("make_perm_golden", os.path.join(GOLDEN, "make_perm_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "rng_permutation.json")) as f:
        return mod, json.load(f)


@_twins(["digests"])
def _permutation(case, mdopt, on_gpu):
    """random_permutation(n) for n = 2048, 2049 (one and two sort tiles), 16385 (a second chunk of the counter scan), 100000: every
    index once, AND the very sequence the double's stable sort of the same Philox keys gives (SHA-256 of the int64 bytes, pinned in
    tests/golden/rng_permutation.json): a mis-sorted result is a permutation too."""
    mod, pinned = _perm_golden()
    assert pinned["seed"] == mod.SEED and pinned["sizes"] == list(mod.SIZES)
    for n, p in zip(mod.SIZES, mod.draw(nd)):
        assert p.dtype == np.int64 and np.array_equal(np.sort(p), np.arange(n)), n
        assert hashlib.sha256(p.tobytes()).hexdigest() == pinned["sha256"][str(n)], n


test_permutation, test_permutation_gpu = _permutation
