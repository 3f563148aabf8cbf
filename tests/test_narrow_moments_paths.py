"""Every launch form of mdhip_var (csrc/moments.hip) on the storage-only dtypes — float16, int8/16, uint8/16/32/64 — and the routes
of nd.mean / nd.std / the statistics' column sums that read such arrays in their own type: the companion of
tests/test_moments_arg_paths.py (whose helpers and data construction this module reuses) for the narrow half of the entry point.

TABLE, as there: what an entry reaches, the array it is cut from, the view, the reduced axis, the dtypes, the edges. Every shape is
derived from the launch predicates with V = 16 bytes / element size (16, 8, 4, 2): var_rows picks by 16-B VECTORS per row (the same
thresholds at every element size — what a thread caches is vectors — so the row lengths in elements scale with V), var_cols needs
inner % V == 0, inner >= 256, n >= 64, outer <= 65535; a strip is 64 lanes x V columns. The calls go through the C-ABI (lib.var) into
a result block filled with 85; test_public_functions runs the same entries through nd.std / nd.mean with keepdims both ways.

  data       the construction of test_moments_arg_paths.py: per output x = m + d, d integers that sum to 0 exactly (small ones at
             random places, larger balanced fours at the edge positions), so the mean is exactly m and q = sum d^2 an exact integer.
             m is chosen so that every element fits the storage type (int8: |m| + max|d| <= 127; unsigned: m - max|d| >= 0;
             float16: integers below 2048, n * max|x| <= 2^24 and q <= 2^24 — every float32 partial sum in any order is exact).
  reference  integers: float64(q) / float64(n - ddof), then np.sqrt. float16: the same in float32, then .astype(float16) — the
             operations the kernel performs. ddof 0 and 1, take_sqrt 0 and 1. At the power-of-two entry (128 x 512, both axes) the
             integer results are also np.std / np.mean's own bits, and np.mean's for the integer-valued float16 data.
  poison     a constant output gives exactly 0; a float16 NaN / +inf in one output makes only that output NaN; outside a view float
             padding is NaN and integer padding the type's maximum (which would wreck the sum).
  uint64     one entry with every element above 2^63 against np.std on the host: relative 8 * 1e-13, the float64 random-data bound
             of tests/test_std_fused.py.
  refusals   the first shape on the far side of each floor, per element size: ValueError from the C-ABI, the result block untouched,
             nd.std still answers (the promote route, today's tolerance). With option var_narrow 0 every accepted entry is refused.
  old route  nd.std with var_narrow 0 (promote -> wide kernel -> demote) and 1 give identical bits on the exact data; on random
             float16 data they agree within one float16 ulp.
  sums       the first pass of the column forms, alone: sum(x, axis, dtype=float64) of the exact integer data and
             sum(x16, axis, dtype=float32) at strips-sized and batched shapes, bit for bit against int64 arithmetic; the whole-array
             mean of int8/16, uint8/16 (k_reduce_all with a float64 accumulator) at 20003 and 8192 elements.
  trace      (CPU double, MDHIP_TRACE) nd.mean of an int8 and of a float16 array issues no `convert` of an operand as large as the
             array.

Each test has a twin: unmarked on the CPU double (skipped when a GPU is bound), gpu-marked on the product library. The double's
mdhip_var knows float32 / float64 alone: its twin asserts the refusal of every entry and checks the integer reference against
np.var in float64; nd.std / nd.mean are exact there too (the promote route meets the same integers)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_moments_arg_paths as B
from minidiff_amd import ndarray as nd

f16, f32, f64 = B.f16, B.f32, B.f64
i8, i16, u8, u16, u32, u64 = B.i8, B.i16, B.u8, B.u16, B.u32, B.u64
BY_SIZE = {1: (i8, u8), 2: (f16, i16, u16), 4: (u32,), 8: (u64,)}
NARROW = tuple(dt for esz in (1, 2, 4, 8) for dt in BY_SIZE[esz])
INTS = tuple(dt for dt in NARROW if dt != f16)
S = slice
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TABLE = []


def _add(id, reaches, base, axis, dtypes, light=False, **k):
    e = B.Entry("nvar-" + id, reaches, base, axis, dtypes, family="var", **k)
    e.light = light
    TABLE.append(e)


# ---- rows: (rows, n) over the last axis, n = nvec * V ---------------------------------------------------------------------------
# <= 128 / 256 / 512 vectors: a wave per row caching 2 / 4 / 8 vectors per lane; <= 1024 / 4096: a block per row caching 4 / 16;
# longer rows are read twice and need >= 256 rows (the "few long rows" floor: outer < 256 and n > 4096 * V). A thread takes vectors
# tig + g * G: the edges are the multiples of G * V elements.
for esz, dts in BY_SIZE.items():
    V = 16 // esz
    for nvec, form, rows in B._ROW_FORMS:
        n, G = nvec * V, 64 if nvec <= 512 else 256
        big = nvec > 4096
        _add(f"rows-{esz}B-{nvec}v", f"k_var_rows {form}, {esz}-byte elements", (rows, n), 1, dts[:1] if big else dts, light=big,
             edges=B._mult(G * V, n, first=3 if big else 99, last=1 if big else 0))
    _add(f"rows-{esz}B-1025x128v", "k_var_rows G=64 NV=2, >= 1024 rows (an odd count: dead waves in the last block)", (1025, 128 * V), 1, dts,
         edges=B._mult(64 * V, 128 * V, first=99, last=0))
    _add(f"rows-{esz}B-padded", "k_var_rows G=64 NV=2, rows 1 .. 7 of 9 (padding above and below)", (9, 65 * V), 1, dts, view=(S(1, 8),),
         edges=B._mult(64 * V, 65 * V, first=99, last=0))


# ---- columns and batched columns --------------------------------------------------------------------------------------------------
def _col_edges(n, inner, outer, V):
    return B._band_edges(n, B._nb_var(n, inner, outer, V), 8)


for esz, dts in BY_SIZE.items():
    V = 16 // esz
    for shape, what in (((64, 256), "inner at the floor, two bands"), ((67, 256 + V), "a partial last strip (clamped lanes), row tail"),
                        ((4099, 256), "64 bands, two batches, with and without tail rows")):
        _add(f"cols-{esz}B-%dx%d" % shape, f"k_var_cols 2-D, {what}", shape, 0, dts, columns=True, edges=_col_edges(shape[0], shape[1], 1, V))
    _add(f"cols-{esz}B-64x4x64", "k_var_cols 2-D, trailing axes collapse into inner = 256", (64, 4, 64), 0, dts, columns=True, edges=_col_edges(64, 256, 1, V))
    for shape, what in (((2, 64, 256), "NB 2"), ((3, 67, 256 + V), "NB 2, partial strip, row tail"), ((5, 200, 512), "NB > 2, the batches share the ticket block")):
        _add(f"batched-{esz}B-" + "x".join(map(str, shape)), f"k_var_cols batched, {what}", shape, 1, dts, columns=True, middle=True,
             edges=_col_edges(shape[1], shape[2], shape[0], V))
    # one band: one block per (strip, batch) already fills the chip — NS * outer == 256
    NS = B._cdiv(256, 64 * V)
    shape = (256 // NS, 64, 256)
    assert B._nb_var(64, 256, shape[0], V) == 1
    _add(f"batched-{esz}B-one-band", "k_var_cols batched, NB 1: no partials, no ticket", shape, 1, dts[:1], light=True, columns=True, middle=True, edges=(4, 32))
    assert B._nb_var(64, 256, 1, V) == 2 and B._nb_var(4099, 256, 1, V) == 64 and B._nb_var(64, 256, 2, V) == 2 and B._nb_var(200, 512, 5, V) > 2
# more strips than ticket words (NS * outer * 16 > 16384): the one-band fallback of var_cols
_add("batched-1B-no-tickets", "k_var_cols batched, 1025 strips in all: one band", (1025, 64, 256), 1, (i8,), light=True, columns=True, middle=True, edges=(4, 32))
# a power-of-two count on both axes: NumPy's own bits (see test_numpy_bits)
_add("pow2-rows", "k_var_rows, n = 512", (128, 512), 1, NARROW, edges=())
_add("pow2-cols", "k_var_cols, n = 128", (128, 512), 0, NARROW, columns=True, edges=lambda dt: _col_edges(128, 512, 1, B._vlen(dt)))

BY_ID = {e.id: e for e in TABLE}
assert len(BY_ID) == len(TABLE)
assert max(int(np.prod(e.base)) for e in TABLE) <= 17 << 20
IDS = [e.id for e in TABLE]


@pytest.fixture(autouse=True)
def eager():
    prev = nd.set_lazy(False)
    yield
    nd.set_lazy(prev)


# ---- data -----------------------------------------------------------------------------------------------------------------------
def _rng(e, dt, salt):
    return np.random.default_rng([1000 + TABLE.index(e), dt.num, salt])


def _out_dtype(dt):
    return f16 if dt == f16 else f64


def _carrier(dt):
    return f32 if dt == f16 else f64


def _data(e, dt, salt=1):
    """(x as rows (n_out, n) of dt, d as int64 rows, m per output, edge positions): test_moments_arg_paths._var_data with the
    mean chosen for the storage type."""
    n, n_out = e.n_red, e.n_out
    rng = _rng(e, dt, salt)
    pos = B._var_positions(e, dt)
    dev = B._edge_devs(len(pos))
    L = n - len(pos)
    half = rng.integers(-3, 4, (n_out, L // 2), dtype=np.int8)
    plain = rng.permuted(np.concatenate([half, -half, np.zeros((n_out, L % 2), dtype=np.int8)], axis=1), axis=1)
    d = np.empty((n_out, n), dtype=np.int16)
    mask = np.zeros(n, dtype=bool)
    mask[pos] = True
    d[:, mask] = dev
    d[:, ~mask] = plain
    dmax = int(np.abs(dev).max(initial=3))
    if dt == f16:
        hi = min(2047, (1 << 24) // n) - dmax
    else:
        hi = min(int(np.iinfo(dt).max), 1 << 36) - dmax           # (n * 2^36 < 2^53: the float64 sums are exact)
    lo = dmax if dt.kind == "u" or dt == f16 else int(np.iinfo(dt).min) + dmax
    o = np.arange(n_out, dtype=np.int64)
    m = hi - (o * 7) % 31 - 2 * ((o // e.inner) % 16)               # another mean in every output, another range in every batch
    assert int(m.min()) >= lo, (e.id, dt.name, lo, hi, dmax)
    q = (d.astype(np.int64) ** 2).sum(axis=1)
    assert (d.sum(axis=1, dtype=np.int64) == 0).all()
    assert dt != f16 or (q.max() <= 1 << 24 and n * (int(m.max()) + dmax) <= 1 << 24)
    x = (m[:, None] + d).astype(dt)
    return x, q, m, pos


def _ref(e, q, dt, ddof, take_sqrt):
    c = _carrier(dt)
    r = q.astype(c) / c.type(e.n_red - ddof)
    assert r.dtype == c
    return (np.sqrt(r) if take_sqrt else r).astype(_out_dtype(dt))


def _direct(d, e, ddof, take_sqrt):
    res = nd.asarray(np.full(B._kshape(e), 85, dtype=_out_dtype(np.dtype(d.dtype))))
    try:
        nd._lib().var(d.desc(), res.desc(), e.axis, ddof, take_sqrt)
    except (ValueError, TypeError):
        assert (res.get() == 85).all(), "a refused call wrote into the result block"
        raise
    return res.get()


def _pad(dt):
    return None if dt == f16 else np.iinfo(dt).max


def _check_entry(e, mdopt, on_gpu):
    for dt in e.dtypes:
        x, q, m, pos = _data(e, dt)
        dev = B._upload(e, B._from_rows(e, x), _pad(dt))
        if not on_gpu:                                              # the double: float32 / float64 alone
            with pytest.raises((ValueError, TypeError)):
                _direct(dev, e, 0, 1)
            if e.n_out * e.n_red <= 1 << 21:
                for ddof in (0, 1):
                    np.testing.assert_allclose(q / (e.n_red - ddof), np.var(x.astype(np.float64), axis=1, ddof=ddof), rtol=1e-12)
            continue
        for ddof in (0, 1):
            for take_sqrt in (0, 1):
                ref = _ref(e, q, dt, ddof, take_sqrt).reshape(B._kshape(e))
                B._equal(_direct(dev, e, ddof, take_sqrt), ref, (e.id, dt.name, "exact", ddof, take_sqrt))
        mdopt("var_narrow", 0)                                      # the A/B switch: refused as before this form existed
        with pytest.raises(ValueError):
            _direct(dev, e, 0, 1)
        mdopt("var_narrow", 1)
        # poison: a constant output; float16: NaN / +inf in one place each of other outputs; the rest keeps its bits
        places = [pos[0], pos[len(pos) // 2], pos[-1]] if pos else [0, e.n_red - 1]
        for bad, take_sqrt in ((np.nan, 1), (np.inf, 0)):
            items = [("const", 0)] + ([("bad", p) for p in dict.fromkeys(places)] if dt == f16 else [])
            for pairs in B._deal(e, dt, items):
                xb = x.copy()
                ref = _ref(e, q, dt, 0, take_sqrt)
                for o, (kind, p) in pairs:
                    if kind == "const":
                        xb[o, :] = m[o]
                        ref[o] = 0
                    else:
                        xb[o, p] = bad
                        ref[o] = np.nan
                keep = B._upload(e, B._from_rows(e, xb), _pad(dt))
                B._equal(_direct(keep, e, 0, take_sqrt), ref.reshape(B._kshape(e)), (e.id, dt.name, "poison", bad, pairs))
            if e.light or dt != f16:
                break


@B._twins(IDS)
def _paths(case, mdopt, on_gpu):
    _check_entry(BY_ID[case], mdopt, on_gpu)


test_narrow_var_paths, test_narrow_var_paths_gpu = _paths


@B._twins(IDS)
def _public_functions(case, mdopt, on_gpu):
    """The same entries through nd.std and nd.mean, keepdims both ways (light entries: the first dtype was the only one). std with
    option var_narrow 0 — the promote route — gives the same bits."""
    e = BY_ID[case]
    for dt in e.dtypes if not e.light else e.dtypes[:1]:
        x, q, m, pos = _data(e, dt, salt=2)
        dev = B._upload(e, B._from_rows(e, x), _pad(dt))
        mean = m.astype(_carrier(dt)).astype(_out_dtype(dt)).reshape(B._kshape(e))
        for keep in (True, False):
            got = nd.mean(dev, axis=e.axis, keepdims=keep).get()
            B._equal(got, mean if keep else mean.squeeze(e.axis), (e.id, dt.name, "mean", keep))
        for ddof in (0, 1):
            ref = _ref(e, q, dt, ddof, 1).reshape(B._kshape(e))
            for keep in (True, False):
                got = nd.std(dev, axis=e.axis, ddof=ddof, keepdims=keep).get()
                B._equal(got, ref if keep else ref.squeeze(e.axis), (e.id, dt.name, ddof, keep))
            if on_gpu and not e.light:
                mdopt("var_narrow", 0)
                old = nd.std(dev, axis=e.axis, ddof=ddof, keepdims=True).get()
                mdopt("var_narrow", 1)
                B._equal(old, ref, (e.id, dt.name, ddof, "var_narrow 0"))


test_narrow_public_functions, test_narrow_public_functions_gpu = _public_functions


@B._twins(["pow2"])
def _numpy_bits(case, mdopt, on_gpu):
    """n a power of two (128 x 512, both axes): the integer results are np.std's and np.mean's own bits (every NumPy intermediate
    is an exact float64 and the divisions are by powers of two or correctly rounded once), and np.mean's for integer-valued float16."""
    for id in ("nvar-pow2-rows", "nvar-pow2-cols"):
        e = BY_ID[id]
        for dt in e.dtypes:
            x, q, m, pos = _data(e, dt, salt=3)
            v = B._from_rows(e, x)
            dev = nd.asarray(v)
            B._equal(nd.mean(dev, axis=e.axis).get(), np.mean(v, axis=e.axis), (id, dt.name, "np.mean"))
            if dt == f16:
                continue
            B._equal(nd.std(dev, axis=e.axis).get(), np.std(v, axis=e.axis), (id, dt.name, "np.std"))
            if on_gpu:
                B._equal(_direct(dev, e, 0, 1), np.std(v, axis=e.axis, keepdims=True), (id, dt.name, "np.std, C-ABI"))


test_numpy_bits, test_numpy_bits_gpu = _numpy_bits


# ---- uint64 above 2^63 ------------------------------------------------------------------------------------------------------------
@B._twins(["uint64"])
def _uint64_upper_half(case, mdopt, on_gpu):
    """Every element >= 2^63 (negative if read as int64): each is converted straight to float64, as np.std does."""
    rng = np.random.default_rng(63)
    for shape, axis in (((67, 258), 0), ((7, 514), 1), ((3, 67, 258), 1)):
        x = (rng.integers(0, 1 << 62, shape, dtype=np.uint64) + np.uint64(1 << 63))
        assert (x.view(np.int64) < 0).all()
        dev = nd.asarray(x)
        ref = np.std(x, axis=axis, keepdims=True)
        assert ref.dtype == f64
        got = [nd.std(dev, axis=axis, keepdims=True).get()]
        if on_gpu:
            res = nd.asarray(np.full(ref.shape, 85, dtype=f64))
            nd._lib().var(dev.desc(), res.desc(), axis, 0, 1)
            got.append(res.get())
        for g in got:
            assert g.dtype == f64 and g.shape == ref.shape
            assert float((np.abs(g - ref) / ref).max()) <= 8 * 1e-13, (shape, axis)


test_uint64_upper_half, test_uint64_upper_half_gpu = _uint64_upper_half


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _refusals(dt):
    V = B._vlen(dt)

    def arr(shape):
        n = int(np.prod(shape))
        return ((np.arange(n, dtype=np.int64) * 7) % 23 + 3).astype(dt).reshape(shape)

    yield "n % V != 0", nd.asarray(arr((8, 64 * V - 1))), 1
    yield "unaligned base", nd.asarray(arr((8 * 64 * V + 16,)))[1:8 * 64 * V + 1].reshape(8, 64 * V), 1
    yield "few long rows", nd.asarray(arr((255, 4096 * V + V))), 1
    yield "column form, n < 64", nd.asarray(arr((63, 256))), 0
    yield "column form, inner < 256", nd.asarray(arr((64, 256 - V))), 0
    yield "column form, inner % V != 0", nd.asarray(arr((64, 256 + V // 2))), 0


@B._twins([dts[0].name for dts in BY_SIZE.values()] + [i16.name])
def _narrow_refusals(case, mdopt, on_gpu):
    """What mdhip_var leaves to the caller at this element size: ValueError from the C-ABI (the double: every narrow x), the result
    block untouched, nd.std answers by the promote route. int8, device only: more than 65535 batches over a middle axis — 65536
    batches of one (64, 256) slab of the exact data, each shifted by its own small integer on the device."""
    dt = np.dtype(case)
    for what, d, axis in _refusals(dt):
        assert d.is_c_contiguous, what
        kshape = tuple(1 if i == axis else n for i, n in enumerate(d.shape))
        res = nd.asarray(np.full(kshape, 85, dtype=_out_dtype(dt)))
        with pytest.raises(ValueError if on_gpu else (ValueError, TypeError)):
            nd._lib().var(d.desc(), res.desc(), axis, 0, 1)
        assert (res.get() == 85).all(), what
        if d.size > 1 << 22 and not on_gpu:                         # (the long rows: the composed route of the double takes seconds)
            continue
        h = d.get()
        for ddof in (0, 1):
            got = nd.std(d, axis=axis, ddof=ddof)
            exp = np.std(h.astype(np.float64), axis=axis, ddof=ddof)
            assert got.dtype == _out_dtype(dt) and got.shape == exp.shape, what
            np.testing.assert_allclose(got.get().astype(np.float64), exp, rtol=1e-3 if dt == f16 else 1e-12, err_msg=what)
    if not on_gpu or dt != i8:
        return
    e = BY_ID["nvar-cols-1B-64x256"]
    x, q, m, pos = _data(e, i8, salt=9)
    slab = np.ascontiguousarray(x.T) - np.int8(40)                  # (64, 256): room for the shifts below the type's maximum
    shift = (np.arange(65536) % 37).astype(i8).reshape(65536, 1, 1)
    big = nd.add(nd.asarray(slab.reshape(1, 64, 256)), nd.asarray(shift))
    assert big.shape == (65536, 64, 256) and big.dtype == i8 and big.is_c_contiguous
    res = nd.asarray(np.full((65536, 1, 256), 85, dtype=f64))
    with pytest.raises(ValueError):
        nd._lib().var(big.desc(), res.desc(), 1, 0, 1)
    assert (res.get() == 85).all()


test_narrow_refusals, test_narrow_refusals_gpu = _narrow_refusals


@B._twins(["dtypes"])
def _wrong_pairings(case, mdopt, on_gpu):
    """Any other x / out pairing is a TypeError (MDHIP_ETYPE), whatever the shape; the block stays untouched."""
    if not on_gpu:
        return
    for xdt, odt in ((i8, f32), (i8, i8), (f16, f32), (f16, f64), (u64, u64), (u32, f32), (f32, f16), (f64, f32)):
        d = nd.asarray(np.ones((64, 256), dtype=xdt))
        res = nd.asarray(np.full((1, 256), 85, dtype=odt))
        with pytest.raises(TypeError):
            nd._lib().var(d.desc(), res.desc(), 0, 0, 1)
        assert (res.get() == 85).all(), (xdt, odt)


test_wrong_pairings, test_wrong_pairings_gpu = _wrong_pairings


# ---- the old route agrees on random float16 data ----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_old_route_agrees_on_random_float16_gpu(lib, on_gpu, mdopt):
    """Both routes compute in float32 and round once; the sums differ in order, so the float32 values differ by a few float32 ulps
    and the float16 results by at most one float16 ulp (a value next to a rounding boundary)."""
    rng = np.random.default_rng(16)
    for shape, axis in (((1025, 1024), 1), ((300, 4104), 1), ((2051, 264), 0), ((5, 200, 512), 1)):
        h = (rng.standard_normal(shape) * 3 + 10).astype(f16)
        dev = nd.asarray(h)
        new = nd.std(dev, axis=axis).get()
        mdopt("var_narrow", 0)
        old = nd.std(dev, axis=axis).get()
        mdopt("var_narrow", 1)
        assert new.dtype == f16 and old.dtype == f16
        ulp = np.spacing(np.maximum(np.abs(new), np.abs(old)).astype(f16)).astype(np.float64)
        assert (np.abs(new.astype(np.float64) - old.astype(np.float64)) <= ulp).all(), (shape, axis)
        ref = np.std(h.astype(np.float64), axis=axis)
        np.testing.assert_allclose(new.astype(np.float64), ref, rtol=2 ** -10)


# ---- the sums of the statistics -----------------------------------------------------------------------------------------------------
def _sum_cases(dt):
    V = B._vlen(dt)
    yield (2051, 1024 + V), 0          # k_reduce_cols_strips with a storage type: >= 512 rows, NS * NB >= 64, a partial last strip
    yield (3, 67, 256 + V), 1          # the batched twin
    yield (5, 200, 512), 1
    yield (300, 256), 0                # under the strips floor: the tiled kernel, as before


@B._twins([dt.name for dt in NARROW])
def _sum_route(case, mdopt, on_gpu):
    """The column sums in NumPy's accumulator for the statistics (float64 for the integers, float32 for float16), read from the
    narrow array: bit for bit against int64 arithmetic (values 0 .. 7: every partial sum is exact in float32 too)."""
    dt = np.dtype(case)
    rng = np.random.default_rng(dt.num)
    acc = _carrier(dt)
    for shape, axis in _sum_cases(dt):
        x = rng.integers(0, 8, shape).astype(dt)
        ref = x.astype(np.int64).sum(axis=axis)
        assert ref.max() < 1 << 24
        for keep in (False, True):
            got = nd.sum(nd.asarray(x), axis=axis, dtype=acc, keepdims=keep).get()
            B._equal(got, (np.expand_dims(ref, axis) if keep else ref).astype(acc), (dt.name, shape, axis, keep))


test_sum_route, test_sum_route_gpu = _sum_route


@B._twins([dt.name for dt in (i8, i16, u8, u16)])
def _whole_array_mean(case, mdopt, on_gpu):
    """mean of the whole array: k_reduce_all with a float64 accumulator over 16-B loads of the narrow type; exact."""
    dt = np.dtype(case)
    rng = np.random.default_rng(dt.num + 100)
    info = np.iinfo(dt)
    for n in (20003, 8192):
        x = rng.integers(info.min, int(info.max) + 1, n).astype(dt)
        x[[0, 4095, 4096, n - 1]] = info.max
        ref = np.float64(int(x.astype(np.int64).sum())) / np.float64(n)
        assert ref == np.mean(x)
        got = nd.mean(nd.asarray(x)).get()
        assert got.dtype == f64 and got.shape == () and got == ref, (dt.name, n, got, ref)
        got = nd.sum(nd.asarray(x), dtype=f64).get()
        assert got.dtype == f64 and got == np.float64(int(x.astype(np.int64).sum())), (dt.name, n)


test_whole_array_mean, test_whole_array_mean_gpu = _whole_array_mean


# ---- trace: no promoted copy --------------------------------------------------------------------------------------------------------
SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from minidiff_amd import _capi
if %(double)r:
    _capi.use_library(%(double)r)
from minidiff_amd import ndarray as nd
rng = np.random.default_rng(0)
a = nd.asarray(rng.integers(-100, 100, (96, 320)).astype(np.int8))
h = nd.asarray(rng.integers(0, 100, (96, 320)).astype(np.float16))
print("BEGIN", flush=True)
r = [nd.mean(a), nd.mean(a, axis=0), nd.mean(a, axis=1, keepdims=True), nd.mean(h), nd.mean(h, axis=0), nd.mean(h, axis=-1)]
r = [x.get() for x in r]
assert r[0].dtype == np.float64 and r[3].dtype == np.float16 and r[4].shape == (320,)
"""


def _mean_trace(tmp_path, on_gpu):
    from conftest import HOST_DOUBLE
    log = tmp_path / "calls.jsonl"
    env = dict(os.environ, MDHIP_TRACE=str(log), MDHIP_LAZY="0")
    p = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT, "double": "" if on_gpu else HOST_DOUBLE}], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    recs = [json.loads(line) for line in log.read_text().splitlines()]
    size = 96 * 320
    sums = [r for r in recs if r["call"] == "reduce"]
    assert len(sums) == 6, [r["call"] for r in recs]
    for r in sums:                                                  # each sum reads the narrow array itself
        assert r["args"][1]["dtype"] in (5, 11) and int(np.prod(r["args"][1]["shape"])) == size, r
    for r in recs:
        if r["call"] == "convert":
            shapes = [int(np.prod(a["shape"])) for a in r["args"] if isinstance(a, dict)]
            assert max(shapes) < size, ("a conversion pass over the operand", r)


def test_mean_issues_no_conversion_pass(tmp_path, lib, on_gpu):
    if on_gpu:
        pytest.skip("other twin")
    _mean_trace(tmp_path, False)


@pytest.mark.gpu
def test_mean_issues_no_conversion_pass_gpu(tmp_path, lib, on_gpu):
    _mean_trace(tmp_path, True)
